// hgx_sets.hip -- the visited sets of many seeds of a finished batched BFS as one CSR (include/hgx_sets.h;
// DESIGN.md 3.10).
//
// The level rows are atom-major (one bit per source, 64 sources a word, W words an atom); the answer is
// source-major.  A wavefront owns a contiguous range of 64-atom tiles.  Per tile and level it tests the tile's
// word of the level bitmap (ANDed with the predicate's word): zero skips the level.  Otherwise lane a loads the
// selected words of atom a's row and the wavefront transposes each 64 x 64 bit block with 64 ballots, so that
// lane b holds the tile's membership mask of source 64 w + b.  The count pass adds population counts into
// cnt[wavefront][column]; a column-wise scan over the wavefronts gives every wavefront its start per source; the
// write pass repeats the transposes and each lane walks its mask, writing ascending atoms at its running
// offset.  Nothing is sorted.
#include "hgx_internal.h"

#include <cstring>
#include <unordered_map>

namespace hgx {
namespace {

constexpr int kTileStride = 65;       // LDS depth tile: 64 atoms x 64 sources, one word of padding a row
constexpr int kMinTilesPerWave = 4;   // a wavefront's contiguous atom range: at least 256 atoms
constexpr int kMaxUnits = 2048;       // wavefronts of one launch (rows of cnt / start)

struct SetsArgs {
    int64_t A, n_tiles;
    int32_t tiles_per_unit, n_units;
    int32_t d0, d1;                  // the levels read: [d0, d1]
    const u64* const* fa;            // [levels] level bitmaps
    const u64* const* lvl;           // [levels] level rows
    const u64* where;                // [A / 64 + 2] or null
    u64 sel[16];                     // per row word: the bits of the selected seeds
    uint32_t* cnt;                   // [n_units][NW * 64] count pass: entries of (wavefront, column)
    const int64_t* start;            // [n_units][NW * 64] write pass: their exclusive scan over the wavefronts
    const int64_t* colbase;          // [NW * 64] write pass: CSR offset of the column's set
    int32_t* atoms;                  // flat output
    int32_t* depths;                 //   (with HGX_SETS_DEPTHS)
    u64* ctr;                        // [2] rows loaded, (tile, level) pairs skipped
};

enum { kCount = 0, kWrite = 1, kWriteDepths = 2 };

// ORs the transpose of the wavefront's 64 x 64 bit block into m: lane b gets bit a set iff lane a's word has bit
// b.  Every lane of the wavefront must be active.
__device__ __forceinline__ void transpose_or(u64 word, int lane, u64& m) {
    if (__ballot(word != 0) == 0) return;   // wave-uniform
    for (int b = 0; b < 64; ++b) {
        const u64 bal = __ballot((word >> b) & 1ull);
        if (lane == b) m |= bal;
    }
}

// The tile's bitmap word at level d: the atoms of the tile whose row is valid, that pass `where`, and that exist.
__device__ __forceinline__ u64 tile_word(const SetsArgs& a, int d, int64_t tile, u64 keep) {
    const u64* f = a.fa[d];
    return f ? f[tile] & keep : 0ull;
}

template <int NW, int MODE>
__global__ void __launch_bounds__(64) hgx_sets_pass(const SetsArgs a) {
    __shared__ int32_t dtile[MODE == kWriteDepths ? 64 * kTileStride : 1];
    const int lane = threadIdx.x;
    const int64_t unit = blockIdx.x;
    const int64_t t0 = unit * a.tiles_per_unit;
    const int64_t t1 = t0 + a.tiles_per_unit < a.n_tiles ? t0 + a.tiles_per_unit : a.n_tiles;
    constexpr int kCols = NW * 64;
    int64_t run[NW];
    uint32_t cnt[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        cnt[w] = 0;
        run[w] = MODE == kCount ? 0 : a.colbase[w * 64 + lane] + a.start[unit * kCols + w * 64 + lane];
    }
    u64 rows = 0, skipped = 0;
    int wfirst = 0;   // the first selected word: it counts the statistics of the depths variant
    while (wfirst < NW - 1 && a.sel[wfirst] == 0) ++wfirst;
    for (int64_t tile = t0; tile < t1; ++tile) {   // wave-uniform
        const int64_t base = tile * 64;
        const int64_t atom = base + lane;
        u64 keep = a.where ? a.where[tile] : ~0ull;
        if (a.A - base < 64) keep &= (1ull << (a.A - base)) - 1ull;   // the last tile: no atom past A
        if constexpr (MODE != kWriteDepths) {
            // one pass over the levels; every selected word of a row is loaded while its line is at hand
            u64 m[NW];
#pragma unroll
            for (int w = 0; w < NW; ++w) m[w] = 0;
            for (int d = a.d0; d <= a.d1; ++d) {
                const u64 fw = tile_word(a, d, tile, keep);
                if (fw == 0) {
                    ++skipped;
                    continue;
                }
                rows += (u64)__popcll(fw);
                const bool on = (fw >> lane) & 1ull;
                const u64* row = a.lvl[d] + atom * NW;
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    if (a.sel[w] == 0) continue;   // wave-uniform
                    transpose_or(on ? row[w] & a.sel[w] : 0ull, lane, m[w]);
                }
            }
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                if (MODE == kCount) {
                    cnt[w] += (uint32_t)__popcll(m[w]);
                } else {
                    u64 mm = m[w];
                    while (mm) {
                        a.atoms[run[w]++] = (int32_t)(base + (__ffsll((unsigned long long)mm) - 1));
                        mm &= mm - 1;
                    }
                }
            }
        } else {
            // one selected word at a time: the depths of its 64 x 64 block go through the LDS tile
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                if (a.sel[w] == 0) continue;   // wave-uniform
                u64 m = 0;
                for (int d = a.d0; d <= a.d1; ++d) {
                    const u64 fw = tile_word(a, d, tile, keep);
                    if (fw == 0) {
                        if (w == wfirst) ++skipped;
                        continue;
                    }
                    if (w == wfirst) rows += (u64)__popcll(fw);
                    u64 word = ((fw >> lane) & 1ull) ? a.lvl[d][atom * NW + w] & a.sel[w] : 0ull;
                    transpose_or(word, lane, m);
                    while (word) {   // the atom side records the depth of each of its hits
                        dtile[lane * kTileStride + (__ffsll((unsigned long long)word) - 1)] = d;
                        word &= word - 1;
                    }
                }
                __syncthreads();   // (one wavefront a block) the tile is written before the source side reads it
                while (m) {
                    const int k = __ffsll((unsigned long long)m) - 1;
                    a.atoms[run[w]] = (int32_t)(base + k);
                    a.depths[run[w]] = dtile[k * kTileStride + lane];
                    ++run[w];
                    m &= m - 1;
                }
                __syncthreads();   // and read before the next block overwrites it
            }
        }
    }
    if (MODE == kCount) {
#pragma unroll
        for (int w = 0; w < NW; ++w) a.cnt[unit * kCols + w * 64 + lane] = cnt[w];
    }
    if (lane == 0) {
        if (rows) atomicAdd(a.ctr, rows);
        if (skipped) atomicAdd(a.ctr + 1, skipped);
    }
}

// Column-wise exclusive scan of cnt over the wavefronts; tot[col] = the column's entries.
__global__ void __launch_bounds__(256) hgx_sets_scan(const uint32_t* __restrict__ cnt, int32_t n_units, int32_t n_cols,
                                                     int64_t* __restrict__ start, int64_t* __restrict__ tot) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= n_cols) return;
    int64_t run = 0;
#pragma unroll 8
    for (int32_t u = 0; u < n_units; ++u) {
        const uint32_t c = cnt[(int64_t)u * n_cols + col];
        start[(int64_t)u * n_cols + col] = run;
        run += c;
    }
    tot[col] = run;
}

template <int NW>
void launch_pass(int mode, const SetsArgs& a, hipStream_t st) {
    if (mode == kCount) hgx_sets_pass<NW, kCount><<<a.n_units, 64, 0, st>>>(a);
    else if (mode == kWrite) hgx_sets_pass<NW, kWrite><<<a.n_units, 64, 0, st>>>(a);
    else hgx_sets_pass<NW, kWriteDepths><<<a.n_units, 64, 0, st>>>(a);
    HGX_CHECK_LAUNCH();
}

void launch_pass(int W, int mode, const SetsArgs& a, hipStream_t st) {
    switch (W) {
        case 1: launch_pass<1>(mode, a, st); break;
        case 2: launch_pass<2>(mode, a, st); break;
        case 4: launch_pass<4>(mode, a, st); break;
        case 8: launch_pass<8>(mode, a, st); break;
        case 16: launch_pass<16>(mode, a, st); break;
        default: fail(HGX_E_DEVICE, "hgx_bfs_result_sets: a batch of " + std::to_string(W) + " row words");
    }
}

// Pool buffers of one call, handed back when it ends (after the stream drained: kernels may still read them on
// an error path).
struct Scratch {
    hgx_graph* g;
    std::vector<PoolBuf> v;
    explicit Scratch(hgx_graph* gg) : g(gg) {}
    template <class T>
    T* get(size_t count) {
        const size_t bytes = sizeof(T) * std::max<size_t>(count, 1);
        void* p = g->alloc(bytes);
        v.push_back({p, bytes});
        return (T*)p;
    }
    template <class T>
    T* upload(const std::vector<T>& h) {
        T* d = get<T>(h.size());
        if (!h.empty()) HGX_HIP(hipMemcpyAsync(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, g->stream));
        return d;
    }
    ~Scratch() {
        (void)hipStreamSynchronize(g->stream);
        for (auto& b : v) g->release(b.p, b.n);
    }
};

// One batch of the result that holds a selected seed the rows engine served.
struct BatchJob {
    int32_t bi = 0, W = 0, d0 = 0, d1 = -1;
    std::vector<int32_t> col_set;   // [W * 64] set index of the column, -1 = not selected
    SetsArgs a{};
    int64_t* start = nullptr;
    int64_t* tot = nullptr;         // (device) [W * 64]
    size_t tot_at = 0;              // its place in the host copy of all totals
};

hipEvent_t take_event(hgx_graph* g) {
    if (!g->ev_pool.empty()) {
        hipEvent_t e = g->ev_pool.back();
        g->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    HGX_HIP(hipEventCreate(&e));
    return e;
}

}  // namespace

void sets_validate(bool have_result, bool have_out, bool shard, int32_t n_result_seeds, const int32_t* seed_index,
                   int32_t n_sets, int32_t min_depth, int32_t max_depth, uint32_t flags) {
    const std::string who = "hgx_bfs_result_sets: ";
    if (!have_result) fail(HGX_E_INVALID, who + "null result");
    if (!have_out) fail(HGX_E_INVALID, who + "null out");
    if (n_sets < 0) fail(HGX_E_INVALID, who + "n_sets " + std::to_string(n_sets) + " is negative");
    if (min_depth < 0) fail(HGX_E_INVALID, who + "min_depth " + std::to_string(min_depth) + " is negative");
    if (max_depth != HGX_UNBOUNDED && max_depth < min_depth)
        fail(HGX_E_INVALID, who + "max_depth " + std::to_string(max_depth) + " is below min_depth " +
                                std::to_string(min_depth));
    if (flags & ~(uint32_t)(HGX_SETS_DEPTHS | HGX_SETS_COUNT_ONLY))
        fail(HGX_E_INVALID, who + "unknown flag bits " + std::to_string(flags));
    if (shard) fail(HGX_E_UNSUPPORTED, who + "the result of a partition shard holds owned atoms only");
    if (n_sets > 0 && !seed_index) fail(HGX_E_INVALID, who + "null seed_index");
    std::unordered_map<int32_t, int32_t> seen;
    seen.reserve((size_t)n_sets);
    for (int32_t i = 0; i < n_sets; ++i) {
        const int32_t s = seed_index[i];
        if (s < 0 || s >= n_result_seeds)
            fail(HGX_E_NOTFOUND, who + "set " + std::to_string(i) + ": no such seed index " + std::to_string(s));
        const auto it = seen.emplace(s, i);
        if (!it.second)
            fail(HGX_E_INVALID, who + "set " + std::to_string(i) + ": seed index " + std::to_string(s) +
                                    " repeats set " + std::to_string(it.first->second));
    }
}

}  // namespace hgx

using namespace hgx;

struct hgx_visited_sets {
    hgx_graph* g = nullptr;
    int32_t n_sets = 0;
    uint32_t flags = 0;
    int64_t total = 0;
    std::vector<int64_t> off;                  // [n_sets + 1]
    // the flat arrays: in pool memory of g when a kernel wrote any of them, else on the host
    bool on_device = false;
    int32_t* d_atoms = nullptr;
    int32_t* d_depths = nullptr;
    std::vector<int32_t> h_atoms, h_depths;
    int64_t rows_read = 0, tiles_skipped = 0, syncs = 0;
    double ms_total = 0, bytes = 0;
    size_t dev_bytes() const { return sizeof(int32_t) * (size_t)std::max<int64_t>(total, 1); }
};

namespace {

// The set of a seed the workgroup stages finished, from its host lists: (atom, depth) ascending by atom.
void host_set(const BlockSet& b, int32_t si, int32_t dmin, int32_t dmax, const std::vector<u64>& keep, bool filtered,
              std::vector<std::pair<int32_t, int32_t>>& out) {
    out.clear();
    auto take = [&](int32_t v, int32_t d) {
        if (filtered && !((keep[(size_t)v >> 6] >> (v & 63)) & 1ull)) return;
        out.emplace_back(v, d);
    };
    if (dmin == 0) take(b.seeds[si], 0);
    int64_t k = 0;
    for (int32_t d = 1; d <= b.levels[si]; ++d) {
        const int64_t e = k + b.lcnt[si][d - 1];
        if (d >= dmin && (dmax < 0 || d <= dmax))
            for (int64_t j = k; j < e; ++j) take(b.atoms[si][j], d);
        k = e;
    }
    std::sort(out.begin(), out.end());
}

void sets_run(hgx_bfs_result* r, const int32_t* seed_index, int32_t n_sets, int32_t min_depth, int32_t max_depth,
              const hgx_atom_predicate* where, uint32_t flags, int64_t max_entries, hgx_visited_sets** out) {
    sets_validate(r != nullptr, out != nullptr, r && r->g->shard, r ? r->n_seeds : 0, seed_index, n_sets, min_depth,
                  max_depth, flags);
    hgx_graph* g = r->g;
    if (where) apred_check(g, where, "hgx_bfs_result_sets");
    struct WhereRef {   // the call's reference on the predicate
        hgx_atom_predicate* p;
        ~WhereRef() { apred_release(p); }
    } wref{apred_ref(const_cast<hgx_atom_predicate*>(where))};
    const bool want_depths = flags & HGX_SETS_DEPTHS, count_only = flags & HGX_SETS_COUNT_ONLY;

    std::unique_ptr<hgx_visited_sets> s(new hgx_visited_sets());
    s->g = g;
    s->n_sets = n_sets;
    s->flags = flags;
    s->off.assign((size_t)n_sets + 1, 0);
    if (n_sets == 0) {
        *out = s.release();
        return;
    }
    std::lock_guard<std::mutex> lk(g->mu);
    HGX_HIP(hipSetDevice(g->device));
    hipStream_t st = g->stream;
    const int64_t A = g->A;
    const size_t bm_words = (size_t)(A / 64 + 2);

    // which engine served each selected seed
    std::vector<int32_t> host_sets;                 // set indices served from the host lists
    std::vector<BatchJob> jobs;
    std::unordered_map<int32_t, size_t> job_of;     // batch -> its job
    for (int32_t i = 0; i < n_sets; ++i) {
        const int32_t si = seed_index[i];
        if (r->blk && r->blk->pairs[si] >= 0) {
            host_sets.push_back(i);
            continue;
        }
        const int32_t ci = r->blk ? r->compact[si] : si;
        const int32_t bi = ci / 1024, bit = ci % 1024;
        auto it = job_of.find(bi);
        if (it == job_of.end()) {
            it = job_of.emplace(bi, jobs.size()).first;
            jobs.emplace_back();
            BatchJob& j = jobs.back();
            const BfsBatch& bt = r->batches[(size_t)bi];
            j.bi = bi;
            j.W = bt.W;
            j.col_set.assign((size_t)bt.W * 64, -1);
            const int32_t nl = (int32_t)bt.lvl.size();
            j.d0 = min_depth;
            j.d1 = max_depth == HGX_UNBOUNDED ? nl - 1 : std::min(max_depth, nl - 1);
        }
        BatchJob& j = jobs[it->second];
        j.col_set[(size_t)bit] = i;
        j.a.sel[bit >> 6] |= 1ull << (bit & 63);
    }

    // the seeds of the host lists: merged, filtered and sorted here
    std::vector<std::vector<std::pair<int32_t, int32_t>>> hsets(host_sets.size());
    std::vector<int64_t> count((size_t)n_sets, 0);
    if (!host_sets.empty()) {
        block_materialize(g, *r->blk);
        std::vector<u64> keep;
        if (where) {   // the predicate's bits, read back once
            keep.resize(bm_words);
            HGX_HIP(hipMemcpyAsync(keep.data(), where->bits, sizeof(u64) * bm_words, hipMemcpyDeviceToHost, st));
            HGX_HIP(hipStreamSynchronize(st));
            ++s->syncs;
        }
        for (size_t k = 0; k < host_sets.size(); ++k) {
            host_set(*r->blk, seed_index[host_sets[k]], min_depth, max_depth, keep, where != nullptr, hsets[k]);
            count[(size_t)host_sets[k]] = (int64_t)hsets[k].size();
        }
    }

    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EvGuard {   // timing events go back to the graph's pool (g->mu is held)
        hgx_graph* g;
        hipEvent_t* ev;
        ~EvGuard() {
            for (int i = 0; i < 2; ++i)
                if (ev[i]) g->ev_pool.push_back(ev[i]);
        }
    } evg{g, ev};
    Scratch sc(g);
    const int64_t n_tiles = ceil_div(A, 64);
    u64* ctr = nullptr;
    std::vector<int64_t> htot;
    int64_t* dtot = nullptr;
    double bytes = 0;
    int64_t pass_cols = 0;
    if (!jobs.empty()) {
        if (g->timing) {
            for (auto& e : ev) e = take_event(g);
            HGX_HIP(hipEventRecord(ev[0], st));
        }
        ctr = sc.get<u64>(2);
        HGX_HIP(hipMemsetAsync(ctr, 0, sizeof(u64) * 2, st));
        size_t n_tot = 0;
        for (BatchJob& j : jobs) {
            j.tot_at = n_tot;
            n_tot += (size_t)j.W * 64;
        }
        dtot = sc.get<int64_t>(n_tot);
        HGX_HIP(hipMemsetAsync(dtot, 0, sizeof(int64_t) * n_tot, st));
        // ---- the count pass and the scan over the wavefronts, one launch pair per batch
        std::vector<std::vector<const u64*>> ptrs(jobs.size());   // (alive until the synchronisation below)
        for (size_t q = 0; q < jobs.size(); ++q) {
            BatchJob& j = jobs[q];
            j.tot = dtot + j.tot_at;
            if (j.d0 > j.d1 || n_tiles == 0) continue;   // no level of the batch is in range: its sets are empty
            const BfsBatch& bt = r->batches[(size_t)j.bi];
            const int32_t nl = (int32_t)bt.lvl.size();
            for (int32_t d = 0; d < nl; ++d) ptrs[q].push_back(bt.fa[(size_t)d]);
            for (int32_t d = 0; d < nl; ++d) ptrs[q].push_back(bt.lvl[(size_t)d]);
            const u64** dp = sc.upload(ptrs[q]);
            SetsArgs& a = j.a;
            a.A = A;
            a.n_tiles = n_tiles;
            a.tiles_per_unit = (int32_t)std::max<int64_t>(kMinTilesPerWave, ceil_div(n_tiles, kMaxUnits));
            a.n_units = (int32_t)ceil_div(n_tiles, a.tiles_per_unit);
            a.d0 = j.d0;
            a.d1 = j.d1;
            a.fa = (const u64* const*)dp;
            a.lvl = (const u64* const*)(dp + nl);
            a.where = where ? where->bits : nullptr;
            const size_t cells = (size_t)a.n_units * j.W * 64;
            a.cnt = sc.get<uint32_t>(cells);
            j.start = sc.get<int64_t>(cells);
            a.start = j.start;
            a.ctr = ctr;
            launch_pass(j.W, kCount, a, st);
            hgx_sets_scan<<<(int)ceil_div(j.W * 64, 256), 256, 0, st>>>(a.cnt, a.n_units, j.W * 64, j.start, j.tot);
            HGX_CHECK_LAUNCH();
            pass_cols += (int64_t)a.n_units * j.W * 64;
        }
        htot.resize(n_tot);
        HGX_HIP(hipMemcpyAsync(htot.data(), dtot, sizeof(int64_t) * n_tot, hipMemcpyDeviceToHost, st));
        HGX_HIP(hipStreamSynchronize(st));   // the sizes (and the pointer tables are uploaded)
        ++s->syncs;
        for (const BatchJob& j : jobs)
            for (size_t c = 0; c < j.col_set.size(); ++c)
                if (j.col_set[c] >= 0) count[(size_t)j.col_set[c]] = htot[j.tot_at + c];
    }

    int64_t total = 0;
    for (int32_t i = 0; i < n_sets; ++i) {
        s->off[(size_t)i] = total;
        total += count[(size_t)i];
    }
    s->off[(size_t)n_sets] = total;
    s->total = total;
    if (max_entries >= 0 && total > max_entries)
        fail(HGX_E_NOMEM, "hgx_bfs_result_sets: the sets hold " + std::to_string(total) + " entries, more than max_entries " +
                              std::to_string(max_entries) + " (page by seeds)");

    bool wrote = false;
    if (!count_only && total > 0) {
        if (jobs.empty()) {   // every seed came from the host lists: no kernel, the arrays stay on the host
            s->h_atoms.resize((size_t)total);
            if (want_depths) s->h_depths.resize((size_t)total);
            for (size_t k = 0; k < host_sets.size(); ++k) {
                int64_t o = s->off[(size_t)host_sets[k]];
                for (const auto& e : hsets[k]) {
                    s->h_atoms[(size_t)o] = e.first;
                    if (want_depths) s->h_depths[(size_t)o] = e.second;
                    ++o;
                }
            }
        } else {
            s->on_device = true;
            s->d_atoms = (int32_t*)g->alloc(s->dev_bytes());
            if (want_depths) s->d_depths = (int32_t*)g->alloc(s->dev_bytes());
            struct OutGuard {   // an error below: the arrays go back to the pool
                hgx_visited_sets* s;
                ~OutGuard() {
                    if (!s) return;
                    if (s->d_atoms) s->g->release(s->d_atoms, s->dev_bytes());
                    if (s->d_depths) s->g->release(s->d_depths, s->dev_bytes());
                    s->d_atoms = s->d_depths = nullptr;
                }
            } og{s.get()};
            // ---- the write pass
            std::vector<std::vector<int64_t>> colbase(jobs.size());
            for (size_t q = 0; q < jobs.size(); ++q) {
                BatchJob& j = jobs[q];
                if (j.d0 > j.d1 || n_tiles == 0) continue;
                colbase[q].assign(j.col_set.size(), 0);
                for (size_t c = 0; c < j.col_set.size(); ++c)
                    if (j.col_set[c] >= 0) colbase[q][c] = s->off[(size_t)j.col_set[c]];
                j.a.colbase = sc.upload(colbase[q]);
                j.a.atoms = s->d_atoms;
                j.a.depths = s->d_depths;
                launch_pass(j.W, want_depths ? kWriteDepths : kWrite, j.a, st);
                wrote = true;
            }
            // the sets of the host lists, spliced in: one copy per run of consecutive sets
            std::vector<int32_t> ha, hd;
            std::vector<std::pair<int64_t, int64_t>> runs;   // (first entry in the flat arrays, first entry in ha)
            for (size_t k = 0; k < host_sets.size(); ++k) {
                if (hsets[k].empty()) continue;
                const int64_t o = s->off[(size_t)host_sets[k]];
                if (runs.empty() || runs.back().first + ((int64_t)ha.size() - runs.back().second) != o)
                    runs.emplace_back(o, (int64_t)ha.size());
                for (const auto& e : hsets[k]) {
                    ha.push_back(e.first);
                    if (want_depths) hd.push_back(e.second);
                }
            }
            for (size_t q = 0; q < runs.size(); ++q) {
                const int64_t n = (q + 1 < runs.size() ? runs[q + 1].second : (int64_t)ha.size()) - runs[q].second;
                HGX_HIP(hipMemcpyAsync(s->d_atoms + runs[q].first, ha.data() + runs[q].second, sizeof(int32_t) * (size_t)n,
                                       hipMemcpyHostToDevice, st));
                if (want_depths)
                    HGX_HIP(hipMemcpyAsync(s->d_depths + runs[q].first, hd.data() + runs[q].second,
                                           sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
            }
            if (ev[1]) HGX_HIP(hipEventRecord(ev[1], st));
            HGX_HIP(hipStreamSynchronize(st));   // the entries are written (and the staging vectors are read)
            ++s->syncs;
            og.s = nullptr;
        }
    }
    if (!jobs.empty()) {
        if (ev[1] && !s->on_device) {
            HGX_HIP(hipEventRecord(ev[1], st));
            HGX_HIP(hipStreamSynchronize(st));
        }
        u64 hc[2] = {0, 0};
        HGX_HIP(hipMemcpy(hc, ctr, sizeof(hc), hipMemcpyDeviceToHost));
        s->rows_read = (int64_t)hc[0];
        s->tiles_skipped = (int64_t)hc[1];
        if (ev[1]) {
            float ms = 0;
            HGX_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
            s->ms_total = ms;
        }
        // algorithmic bytes: per pass the bitmap (and predicate) word of every (tile, level) pair and the selected
        // words of the rows loaded; the counts written, scanned and read back; the offsets; the entries written
        int64_t sel_words = 0, pairs = 0;
        for (const BatchJob& j : jobs) {
            if (j.d0 > j.d1) continue;
            int32_t nsel = 0;
            for (int w = 0; w < j.W; ++w) nsel += j.a.sel[w] != 0;
            sel_words = std::max<int64_t>(sel_words, nsel);
            pairs += n_tiles * (int64_t)(j.d1 - j.d0 + 1);
        }
        const double passes = wrote ? 2 : 1;
        bytes += passes * (double)pairs * (where ? 16 : 8);
        bytes += (double)hc[0] * 8 * (double)sel_words;   // (rows_read already covers both passes)
        bytes += (double)pass_cols * (4 + 4 + 8) + (wrote ? (double)pass_cols * 8 : 0);
    }
    bytes += 8.0 * (n_sets + 1);
    if (!count_only) bytes += (double)total * (want_depths ? 8 : 4);
    s->bytes = bytes;
    *out = s.release();
}

}  // namespace

extern "C" {

int hgx_bfs_result_sets(hgx_bfs_result* r, const int32_t* seed_index, int32_t n_sets, int32_t min_depth,
                        int32_t max_depth, const hgx_atom_predicate* where, uint32_t flags, int64_t max_entries,
                        hgx_visited_sets** out) {
    HGX_API_BEGIN
    sets_run(r, seed_index, n_sets, min_depth, max_depth, where, flags, max_entries, out);
    HGX_API_END
}

int hgx_visited_sets_info(const hgx_visited_sets* s, int32_t* n_sets, int64_t* total, uint32_t* flags) {
    HGX_API_BEGIN
    if (!s) fail(HGX_E_INVALID, "hgx_visited_sets_info: null sets");
    if (n_sets) *n_sets = s->n_sets;
    if (total) *total = s->total;
    if (flags) *flags = s->flags;
    HGX_API_END
}

int hgx_visited_sets_offsets(const hgx_visited_sets* s, int64_t* off) {
    HGX_API_BEGIN
    if (!s || !off) fail(HGX_E_INVALID, "hgx_visited_sets_offsets: bad argument");
    std::memcpy(off, s->off.data(), sizeof(int64_t) * s->off.size());
    HGX_API_END
}

int hgx_visited_sets_read(const hgx_visited_sets* s, int64_t first, int64_t n, int32_t* atoms, int32_t* depths) {
    HGX_API_BEGIN
    if (!s) fail(HGX_E_INVALID, "hgx_visited_sets_read: null sets");
    if (s->flags & HGX_SETS_COUNT_ONLY) fail(HGX_E_INVALID, "hgx_visited_sets_read: the object was made count-only");
    if (depths && !(s->flags & HGX_SETS_DEPTHS))
        fail(HGX_E_INVALID, "hgx_visited_sets_read: the object was made without HGX_SETS_DEPTHS");
    if (first < 0 || n < 0 || first > s->total) fail(HGX_E_INVALID, "hgx_visited_sets_read: entry range out of bounds");
    const size_t k = (size_t)std::min(n, s->total - first);
    if (k == 0) return HGX_OK;
    if (!s->on_device) {
        if (atoms) std::memcpy(atoms, s->h_atoms.data() + first, sizeof(int32_t) * k);
        if (depths) std::memcpy(depths, s->h_depths.data() + first, sizeof(int32_t) * k);
        return HGX_OK;
    }
    hgx_graph* g = s->g;
    std::lock_guard<std::mutex> lk(g->mu);
    HGX_HIP(hipSetDevice(g->device));
    if (atoms)
        HGX_HIP(hipMemcpyAsync(atoms, s->d_atoms + first, sizeof(int32_t) * k, hipMemcpyDeviceToHost, g->stream));
    if (depths)
        HGX_HIP(hipMemcpyAsync(depths, s->d_depths + first, sizeof(int32_t) * k, hipMemcpyDeviceToHost, g->stream));
    HGX_HIP(hipStreamSynchronize(g->stream));
    HGX_API_END
}

int hgx_visited_sets_stats(const hgx_visited_sets* s, int64_t* rows_read, int64_t* tiles_skipped, double* ms_total,
                           double* bytes) {
    HGX_API_BEGIN
    if (!s) fail(HGX_E_INVALID, "hgx_visited_sets_stats: null sets");
    if (rows_read) *rows_read = s->rows_read;
    if (tiles_skipped) *tiles_skipped = s->tiles_skipped;
    if (ms_total) *ms_total = s->ms_total;
    if (bytes) *bytes = s->bytes;
    HGX_API_END
}

void hgx_visited_sets_free(hgx_visited_sets* s) {
    if (!s) return;
    if (s->on_device) {   // the arrays go back to the graph's pool
        std::lock_guard<std::mutex> lk(s->g->mu);
        if (s->d_atoms) s->g->release(s->d_atoms, s->dev_bytes());
        if (s->d_depths) s->g->release(s->d_depths, s->dev_bytes());
    }
    delete s;
}

}  // extern "C"
