// hgx_scan.hip -- clauses without an incidence anchor: a scan of the type index (hgx_pattern_batch_dnf_scan).
//
// Replaces the plan AndToQuery.getQuery (C/query/cond2qry/AndToQuery.java:120-294) makes for an And whose only
// ordered set is its type condition: a scan of indexByType.find(T) wrapped in one PredicateBasedFilter per
// remaining condition (:279-294) -- ArityCondition.satisfies, OrderedLinkCondition.satisfies on all-ANY
// patterns, Not.satisfies.  That is a stream over one segment of a sorted index, a predicate per row and an
// order-preserving compaction.
//
// The type index (ensure_type_index): one 16-byte record per link row -- (link atom, arity, first target
// offset) -- the rows stably sorted by link_type, so a type is one segment whose atoms ascend.  The sorted
// distinct keys with their segment offsets live on the host: the host knows every scanned clause's segment and
// sizes the stage exactly.  No table is sized by the largest key.
//
// GPU formulation: the scanned clauses' segments cut into one flat space of 64-entry chunks.
//   hgx_scan_eval    -- a wave per chunk (each wave walks a contiguous range of them, the next chunk's records
//        loading while this one's are tested), a lane per index entry: arity, minimum arity, then the clause's
//        negations on the row it holds (the walk and the leaves of hgx_not_dev.h; all 64 lanes belong to one
//        clause, so the program reads are wave-uniform).  Targets are loaded only when a literal of the
//        clause reads them; the clause's type is known from the segment, so link_type is never read.  One
//        ballot gives the chunk's keep word and count.  Over the atom index (hgx_atoms.hip) the
//        ATOMS instantiation walks a node record's negations by the node rules of include/hgx_atoms.h;
//   the scan         -- cpre = exclusive prefix sum of the chunk counts (rocPRIM);
//   hgx_scan_offsets -- the merged run offsets (the clause stage's + the scanned rows kept before each clause)
//        and the workspace check: anchored + scanned hits beyond the capacity set the clause stage's overflow
//        word and the needed total, every later kernel returns at once and the host runs the batch again;
//   hgx_scan_move    -- a lane per anchored hit: to its place in the merged hit space (only when the batch has
//        an anchored clause);
//   hgx_scan_emit    -- a wave per chunk: a kept lane writes its atom to the clause's run start + the chunk's
//        prefix inside the clause + the kept lanes below it.  No atomic decides a position.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>

#include "hgx_not_dev.h"

namespace hgx {

namespace {

__global__ void __launch_bounds__(256) k_ti_iota(int64_t M, int32_t* __restrict__ row) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (int64_t)gridDim.x * blockDim.x)
        row[i] = (int32_t)i;
}

__global__ void __launch_bounds__(256) k_ti_fill(int64_t M, const int32_t* __restrict__ row,
                                                 const int32_t* __restrict__ link_atom,
                                                 const int64_t* __restrict__ tgt_off, int4* __restrict__ idx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t r = row[i];
        const int64_t b = tgt_off[r], e = tgt_off[r + 1];
        idx[i] = make_int4(link_atom[r], (int32_t)(e - b), (int32_t)(uint32_t)(b & 0xffffffffll), (int32_t)(b >> 32));
    }
}

// The scanned clause a chunk belongs to.  A wave walks a contiguous range of chunks: one binary search at its
// first chunk, then a step to the next descriptor whenever a chunk passes the clause's last (every descriptor
// owns at least one chunk, so chunk_beg ascends strictly).
struct ScanCursor {
    int64_t k, cb, ce;   // descriptor, its first chunk, the next descriptor's first chunk
    ScanDesc d;
};
__device__ __forceinline__ void cursor_at(const ScanArgs& a, int64_t ch, ScanCursor& c) {
    c.k = upper_bound_off(a.chunk_beg, (int64_t)a.n_scan + 1, ch) - 1;
    c.cb = a.chunk_beg[c.k];
    c.ce = a.chunk_beg[c.k + 1];
    c.d = a.desc[c.k];
}
__device__ __forceinline__ void cursor_step(const ScanArgs& a, int64_t ch, ScanCursor& c) {   // ch = the previous chunk + 1
    if (ch < c.ce) return;
    ++c.k;
    c.cb = c.ce;
    c.ce = a.chunk_beg[c.k + 1];
    c.d = a.desc[c.k];
}
// chunks [c0, c1) of wave w among nw
__device__ __forceinline__ void wave_range(int64_t n_chunks, int64_t& c0, int64_t& c1) {
    const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t per = (n_chunks + nw - 1) / nw;
    c0 = w * per < n_chunks ? w * per : n_chunks;
    c1 = c0 + per < n_chunks ? c0 + per : n_chunks;
}

// ATOMS: a.idx is the atom index (hgx_atoms.hip); a node record (high offset word kAtomNode, arity 0) walks its
// negations by the node rules of include/hgx_atoms.h.  The link index runs the instantiation without the branch.
template <bool ATOMS>
__global__ void __launch_bounds__(256) hgx_scan_eval(ScanArgs a) {
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.cnt[a.n_chunks] = 0;
    int64_t c0, c1;
    wave_range(a.n_chunks, c0, c1);   // (the range depends on the wave alone: every lane takes every trip)
    u64 kept = 0, targets_read = 0, walked = 0, types_read = 0;
    if (c0 < c1) {
        ScanCursor c;
        cursor_at(a, c0, c);
        int64_t i = (c0 - c.cb) * 64 + lane;
        bool valid = i < c.d.seg_len;
        int4 rec = make_int4(0, 0, 0, 0);
        if (valid) rec = a.idx[c.d.seg_beg + i];
        for (int64_t ch = c0; ch < c1; ++ch) {
            const ScanDesc d = c.d;
            const int4 cur = rec;
            bool keep = valid;
            if (ch + 1 < c1) {   // the next chunk's record is on its way while this one is tested
                cursor_step(a, ch + 1, c);
                i = (ch + 1 - c.cb) * 64 + lane;
                valid = i < c.d.seg_len;
                if (valid) rec = a.idx[c.d.seg_beg + i];
            }
            if (keep) {
                keep = (d.arity < 0 || cur.y == d.arity) && cur.y >= d.min_arity;
                if (ATOMS && keep && d.g0 < d.g1 && cur.w == kAtomNode) {
                    ++walked;
                    Link L;
                    L.n = 0;
                    L.tg = nullptr;
                    int32_t type = d.type;
                    keep = negations_keep<true>(a.prog, d.g0, d.g1, L, nullptr, 0, type, types_read);
                } else if (keep && d.g0 < d.g1) {
                    ++walked;
                    Link L;
                    L.n = cur.y;
                    L.tg = a.tgt_idx + ((int64_t)(uint32_t)cur.z | ((int64_t)cur.w << 32));
                    if (d.needs_targets) {
#pragma unroll
                        for (int t = 0; t < 8; ++t) L.r[t] = t < L.n ? L.tg[t] : -1;
                        targets_read += (u64)L.n;
                    } else {
#pragma unroll
                        for (int t = 0; t < 8; ++t) L.r[t] = -1;
                    }
                    int32_t type = d.type;   // known from the segment: a type literal reads no link_type
                    keep = negations_keep(a.prog, d.g0, d.g1, L, nullptr, 0, type, types_read);
                }
            }
            const u64 word = __ballot(keep);
            if (lane == 0) {
                a.word[ch] = word;
                a.cnt[ch] = (int64_t)__popcll(word);
            }
            kept += keep ? 1 : 0;
        }
    }
    wave_add(a.ctr + 0, kept);
    wave_add(a.ctr + 1, targets_read);
    wave_add(a.ctr + 2, walked);
}

__global__ void __launch_bounds__(256) hgx_scan_offsets(ScanArgs a) {
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, ts = (int64_t)gridDim.x * blockDim.x;
    // (after an overflow of the clause stage run_in holds nothing meaningful; nobody reads run_out then)
    for (int64_t c = t0; c <= a.n_clauses; c += ts) a.run_out[c] = a.run_in[c] + a.cpre[a.clause_chunk[c]];
    if (t0 == 0) {   // the only reader and writer of the overflow word in this kernel
        const int64_t S = a.cpre[a.n_chunks];
        if (a.stat[2]) {
            a.stat[1] += S;   // the clause stage asked for its candidates: the scanned rows on top
        } else {
            const int64_t tot = a.run_in[a.n_clauses] + S;
            if (tot > a.cap) {
                a.stat[2] = 1;
                if (a.stat[1] < tot) a.stat[1] = tot;
            }
        }
    }
}

__global__ void __launch_bounds__(256) hgx_scan_move(ScanArgs a) {
    if (a.stat[2]) return;
    const int64_t H = a.run_in[a.n_clauses];
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < H; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = upper_bound_off(a.run_in, (int64_t)a.n_clauses + 1, e) - 1;
        a.hits_out[a.run_out[c] + (e - a.run_in[c])] = a.hits_in[e];
    }
}

__global__ void __launch_bounds__(256) hgx_scan_emit(ScanArgs a) {
    if (a.stat[2]) return;
    const int lane = threadIdx.x & 63;
    int64_t c0, c1;
    wave_range(a.n_chunks, c0, c1);
    if (c0 < c1) {
        ScanCursor c;
        cursor_at(a, c0, c);
        for (int64_t ch = c0; ch < c1; ++ch) {
            cursor_step(a, ch, c);
            const u64 word = a.word[ch];
            if (!((word >> lane) & 1ull)) continue;
            const int64_t slot = a.run_out[c.d.clause] + (a.cpre[ch] - a.cpre[c.cb]) +
                                 (int64_t)__popcll(word & ((1ull << lane) - 1ull));
            a.hits_out[slot] = a.idx[c.d.seg_beg + (ch - c.cb) * 64 + lane].x;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) a.out_ctr[threadIdx.x] = a.ctr[threadIdx.x];
}

}  // namespace

void drop_type_index(hgx_graph* g) {
    if (g->type_idx && (!g->base || g->type_idx != g->base->type_idx)) (void)hipFree(g->type_idx);
    g->type_idx = nullptr;
    g->type_idx_built = false;
    g->type_key.clear();
    g->type_seg.clear();
}

void ensure_type_index(hgx_graph* g) {
    if (g->type_idx_built) return;
    if (g->base) {   // an execution context: the snapshot builds the index once and every context borrows it
        hgx_graph* b = g->base;
        std::lock_guard<std::mutex> lk(b->mu);   // lock order: context, then its snapshot (never the reverse)
        HGX_HIP(hipSetDevice(b->device));
        ensure_type_index(b);
        g->type_idx = b->type_idx;
        g->type_key = b->type_key;
        g->type_seg = b->type_seg;
        g->type_idx_built = true;
        return;
    }
    const int64_t M = g->M;
    g->type_key.clear();
    g->type_seg.assign(1, 0);
    if (M == 0) {
        g->type_idx_built = true;
        return;
    }
    hipStream_t s = g->stream;
    PoolScratch sc{g, {}};
    int32_t* row = (int32_t*)sc.take(sizeof(int32_t) * M);
    int32_t* row2 = (int32_t*)sc.take(sizeof(int32_t) * M);
    int32_t* key2 = (int32_t*)sc.take(sizeof(int32_t) * M);
    int32_t* uniq = (int32_t*)sc.take(sizeof(int32_t) * M);
    unsigned int* cnt = (unsigned int*)sc.take(sizeof(unsigned int) * M);
    int64_t* nruns = (int64_t*)sc.take(sizeof(int64_t));
    k_ti_iota<<<grid_for(M, 256, 4096), 256, 0, s>>>(M, row);
    HGX_CHECK_LAUNCH();
    // a radix sort is stable: inside a type the rows stay ascending (signed 32-bit keys)
    size_t tb = 0;
    HGX_HIP(rocprim::radix_sort_pairs(nullptr, tb, g->link_type, key2, row, row2, (size_t)M, 0u, 32u, s));
    void* tmp = sc.take(tb);
    HGX_HIP(rocprim::radix_sort_pairs(tmp, tb, g->link_type, key2, row, row2, (size_t)M, 0u, 32u, s));
    size_t rb = 0;
    HGX_HIP(rocprim::run_length_encode(nullptr, rb, key2, (unsigned int)M, uniq, cnt, nruns, s));
    void* rtmp = sc.take(rb);
    HGX_HIP(rocprim::run_length_encode(rtmp, rb, key2, (unsigned int)M, uniq, cnt, nruns, s));
    int4* idx = nullptr;
    HGX_HIP(hipMalloc(&idx, sizeof(int4) * (size_t)M));
    struct Guard {
        int4* p;
        ~Guard() { if (p) (void)hipFree(p); }
    } guard{idx};
    k_ti_fill<<<grid_for(M, 256, 4096), 256, 0, s>>>(M, row2, g->link_atom, g->tgt_off, idx);
    HGX_CHECK_LAUNCH();
    int64_t nr = 0;
    HGX_HIP(hipMemcpyAsync(&nr, nruns, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HGX_HIP(hipStreamSynchronize(s));
    if (nr < 1 || nr > M) fail(HGX_E_DEVICE, "type index: bad histogram");
    std::vector<unsigned int> hc((size_t)nr);
    g->type_key.resize((size_t)nr);
    HGX_HIP(hipMemcpyAsync(g->type_key.data(), uniq, sizeof(int32_t) * (size_t)nr, hipMemcpyDeviceToHost, s));
    HGX_HIP(hipMemcpyAsync(hc.data(), cnt, sizeof(unsigned int) * (size_t)nr, hipMemcpyDeviceToHost, s));
    HGX_HIP(hipStreamSynchronize(s));
    g->type_seg.resize((size_t)nr + 1);
    for (int64_t i = 0; i < nr; ++i) g->type_seg[i + 1] = g->type_seg[i] + (int64_t)hc[i];
    if (g->type_seg[nr] != M) {
        g->type_key.clear();
        g->type_seg.assign(1, 0);
        fail(HGX_E_DEVICE, "type index: the histogram does not cover the links");
    }
    g->type_idx = idx;
    guard.p = nullptr;
    g->type_idx_built = true;
}

size_t scan_temp_bytes(int64_t n_chunks, hipStream_t s) {
    size_t sb = 0;
    HGX_HIP(rocprim::exclusive_scan(nullptr, sb, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0,
                                    (size_t)n_chunks + 1, rocprim::plus<int64_t>(), s));
    return sb;
}

void scan_launch(const ScanArgs& a, hipStream_t s, bool atoms) {
    HGX_HIP(hipMemsetAsync(a.ctr, 0, sizeof(u64) * 8, s));
    const int wgrid = grid_for(a.n_chunks * 64, 256, 4096);
    if (atoms) hgx_scan_eval<true><<<wgrid, 256, 0, s>>>(a);
    else hgx_scan_eval<false><<<wgrid, 256, 0, s>>>(a);
    HGX_CHECK_LAUNCH();
    size_t sb = a.tmp_bytes;
    HGX_HIP(rocprim::exclusive_scan(a.tmp, sb, (const int64_t*)a.cnt, a.cpre, (int64_t)0, (size_t)a.n_chunks + 1,
                                    rocprim::plus<int64_t>(), s));
    hgx_scan_offsets<<<grid_for((int64_t)a.n_clauses + 1, 256, 1024), 256, 0, s>>>(a);
    HGX_CHECK_LAUNCH();
    if (a.move) {
        hgx_scan_move<<<grid_for(a.cap, 256, 4096), 256, 0, s>>>(a);
        HGX_CHECK_LAUNCH();
    }
    hgx_scan_emit<<<wgrid, 256, 0, s>>>(a);
    HGX_CHECK_LAUNCH();
}

}  // namespace hgx

using namespace hgx;

extern "C" int hgx_graph_type_links(hgx_graph* g, const int32_t* types, int64_t n, int64_t* out_counts) {
    HGX_API_BEGIN
    if (!g || n < 0 || (n > 0 && (!types || !out_counts))) fail(HGX_E_INVALID, "hgx_graph_type_links: bad argument");
    if (g->shard) fail(HGX_E_UNSUPPORTED, "hgx_graph_type_links: not available on a partition shard");
    std::lock_guard<std::mutex> lk(g->mu);
    HGX_HIP(hipSetDevice(g->device));
    ensure_type_index(g);
    for (int64_t i = 0; i < n; ++i) {
        const auto it = std::lower_bound(g->type_key.begin(), g->type_key.end(), types[i]);
        const size_t k = (size_t)(it - g->type_key.begin());
        out_counts[i] = (it != g->type_key.end() && *it == types[i]) ? g->type_seg[k + 1] - g->type_seg[k] : 0;
    }
    HGX_API_END
}
