// hgx_hops.hip -- shortest hop paths and predecessor rows out of a finished batched BFS (include/hgx_hops.h).
//
// Replaces the 3-argument GraphClassics.dijkstra (C/algorithms/GraphClassics.java:80-83: every link weighs
// 1.0) for many (start, goal) pairs at once.  With unit weights an atom's distance is its BFS depth and rule R
// of hgx_paths.h is the reference's final predecessorMatrix entry:
//
//   pred(n), n at depth d >= 1  =  the lowest-rank atom a != n of level d - 1 whose generate(a) yields n,
//                                  with the lowest link atom among a's qualifying links to n
//
// so a finished hgx_bfs_result already holds every shortest path; what is computed here is the backtrace:
//
//   hgx_hop_depth   per pair, the level of the goal (hops)
//   hgx_hop_step    launch k: for every pair with hops >= k, the predecessor of its current node -- a walk
//                   of the node's incidence entries (a lane per entry), the REVERSE generator rule per
//                   co-target, a membership probe of level d - 1, a wavefront minimum and one atomicMin
//   hgx_hop_write   keys -> flat atom / link arrays
//   hgx_hop_depth_row / hgx_hop_pred_row / hgx_hop_pred_heavy   the same for every atom of one seed
//
// Membership of atom a in level d of a seed has two forms: the rows engine's level rows (bit a of fa[d],
// then the seed's bit of row a of lvl[d] -- rows are valid only behind the fa bit), and, for seeds the
// workgroup / grid stages finished, a sorted (atom, depth) table probed by binary search.
//
// Reverse rule.  In a link with targets T that holds n at first / last position fn / ln, atom a (first /
// last position fa / la) yields n iff (pyref.reachable(mode, T, a, n)):
//   symmetric: always;  after-first: fa < ln;  before-first: fa > fn;  before-last: la > fn;  after-last: la < ln.

#include <cstring>
#include <type_traits>
#include <unordered_map>

#include "hgx_internal.h"

namespace hgx {
namespace {

constexpr u64 kNoKey = ~0ull;

// Device words of one call.
enum { cEntries = 0, cPins = 1, cFaProbes = 2, cRowProbes = 3, cWords = 8 };

struct HopGraph {
    int64_t A;
    int32_t mode, want_type;
    const int64_t* inc_off;
    const int32_t* inc_row;
    const int32_t* inc_type;
    const int64_t* tgt_off;
    const int32_t* tgt_idx;
    const int32_t* link_atom;
};

// One requested seed: its level rows (rows engine) or its (atom << 32 | depth) table, ascending.
struct HopSeed {
    const u64* const* fa;    // [nlev] level bitmaps
    const u64* const* lvl;   // [nlev] level rows, A x W words each
    const u64* tab;          // [n_tab]
    int32_t nlev, W, bit, n_tab;
};

struct Counts {
    u64 entries = 0, pins = 0, fa = 0, row = 0;
};

// The rows engine's membership test: the fa word first (A / 8 bytes a level, cache resident), the 8-byte row
// word only behind a set fa bit.
struct RowsMember {
    __device__ static bool in_level(const HopSeed& s, int32_t d, int32_t a, Counts& c) {
        if (d < 0 || d >= s.nlev) return false;
        ++c.fa;
        if (!((s.fa[d][a >> 6] >> (a & 63)) & 1ull)) return false;
        ++c.row;
        return (s.lvl[d][(int64_t)a * s.W + (s.bit >> 6)] >> (s.bit & 63)) & 1ull;
    }
    __device__ static int32_t depth_of(const HopSeed& s, int32_t a, Counts& c) {
        for (int32_t d = 0; d < s.nlev; ++d)
            if (in_level(s, d, a, c)) return d;
        return -1;
    }
};

// The table form (workgroup / grid-stage seeds): binary search of the seed's sorted (atom, depth) keys.
struct TableMember {
    __device__ static int32_t depth_of(const HopSeed& s, int32_t a, Counts& c) {
        int32_t lo = 0, hi = s.n_tab;
        const u64 want = (u64)(uint32_t)a << 32;
        ++c.fa;
        while (lo < hi) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            ++c.row;
            if (s.tab[mid] < want) lo = mid + 1;
            else hi = mid;
        }
        if (lo < s.n_tab) {
            const u64 k = s.tab[lo];
            if ((k >> 32) == (u64)(uint32_t)a) return (int32_t)(uint32_t)k;
        }
        return -1;
    }
    __device__ static bool in_level(const HopSeed& s, int32_t d, int32_t a, Counts& c) { return depth_of(s, a, c) == d; }
};

// Sum / minimum over the wavefront.  Every lane of the wavefront must be active (call at a wave-uniform
// point): a shuffle that reads an inactive lane returns garbage.
__device__ __forceinline__ u64 wave_min(u64 v) {
    for (int o = 32; o > 0; o >>= 1) {
        const u64 w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ u64 wave_sum(u64 v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ void wave_count(u64* ctr, const Counts& c, int lane) {
    const u64 e = wave_sum(c.entries), p = wave_sum(c.pins), f = wave_sum(c.fa), r = wave_sum(c.row);
    if (lane == 0 && (e | p | f | r)) {
        atomicAdd(ctr + cEntries, e);
        atomicAdd(ctr + cPins, p);
        atomicAdd(ctr + cFaProbes, f);
        atomicAdd(ctr + cRowProbes, r);
    }
}

// One incidence entry ei of the current node n: the least key (a << 32 | link atom) over the co-targets a of
// its link that yield n (the reverse rule above) and pass ok(a); kNoKey when there is none.
template <class Ok>
__device__ __forceinline__ u64 hop_entry(const HopGraph& g, int32_t n, int64_t ei, Counts& c, Ok ok) {
    ++c.entries;
    if (g.want_type >= 0 && g.inc_type[ei] != g.want_type) return kNoKey;   // linkPredicate (DefaultALGenerator.java:300-308)
    const int32_t row = g.inc_row[ei];
    const int64_t p = g.tgt_off[row], pe = g.tgt_off[row + 1];
    int64_t lo = p, hi = pe;     // candidate positions
    int64_t xlo = 0, xhi = 0;    // a candidate must not occur in [xlo, xhi)
    if (g.mode != kSym) {
        int64_t fn = -1, ln = -1;
        for (int64_t q = p; q < pe; ++q)
            if (g.tgt_idx[q] == n) {
                if (fn < 0) fn = q;
                ln = q;
            }
        c.pins += (u64)(pe - p);
        if (fn < 0) return kNoKey;
        if (g.mode == kAfterFirst) hi = ln;              // first(a) < last(n)
        else if (g.mode == kBeforeLast) lo = fn + 1;     // last(a) > first(n)
        else if (g.mode == kBeforeFirst) {               // first(a) > first(n): a nowhere before it
            lo = fn + 1;
            xlo = p;
            xhi = fn;
        } else {                                         // last(a) < last(n): a nowhere after it
            hi = ln;
            xlo = ln + 1;
            xhi = pe;
        }
    }
    u64 best = kNoKey;
    const u64 link = (u64)(uint32_t)g.link_atom[row];
    for (int64_t q = lo; q < hi; ++q) {
        const int32_t t = g.tgt_idx[q];
        ++c.pins;
        if (t == n) continue;
        if (best != kNoKey && (u64)(uint32_t)t >= (best >> 32)) continue;   // cannot lower the key
        bool excluded = false;
        for (int64_t x = xlo; x < xhi && !excluded; ++x) {
            excluded = g.tgt_idx[x] == t;
            ++c.pins;
        }
        if (excluded) continue;
        if (ok(t)) best = ((u64)(uint32_t)t << 32) | link;
    }
    return best;
}

struct HopArgs {
    HopGraph g;
    const HopSeed* seeds;        // [distinct requested seeds]
    const int32_t* pair_seed;    // [n_pairs] index into seeds
    const int32_t* goal;         // [n_pairs]
    int32_t* hops;               // [n_pairs]
    const int64_t* off;          // [n_pairs + 1] atom offsets
    const int64_t* loff;         // [n_pairs] link offsets
    u64* key;                    // [total atoms] key[off[i] + j] = (atom j of the path << 32) | link to atom j + 1
    u64* ctr;
    const int32_t* list;         // the pairs of this launch's membership kind
    int32_t n_list;
    int32_t k;                   // step number (hgx_hop_step)
};

// hops[pair] = the level of the goal: one wavefront per pair, a lane per level (rows) or one search (table).
template <class M>
__global__ void __launch_bounds__(256) hgx_hop_depth(HopArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    if (wave >= a.n_list) return;   // wave-uniform
    const int32_t pair = a.list[wave];
    const HopSeed s = a.seeds[a.pair_seed[pair]];
    const int32_t goal = a.goal[pair];
    Counts c;
    int32_t res = -1;
    if constexpr (std::is_same<M, RowsMember>::value) {
        for (int32_t d0 = 0; d0 < s.nlev; d0 += 64) {   // wave-uniform trip count and exit
            const int32_t d = d0 + lane;
            const bool hit = d < s.nlev && M::in_level(s, d, goal, c);
            const u64 m = __ballot(hit);
            if (m) {
                res = d0 + __ffsll((long long)m) - 1;
                break;
            }
        }
    } else {
        Counts mine;
        res = M::depth_of(s, goal, mine);   // every lane the same search; lane 0 counts it
        if (lane == 0) c = mine;
    }
    if (lane == 0) a.hops[pair] = res;
    wave_count(a.ctr, c, lane);
}

// The goal ends every reached pair's key row.
__global__ void __launch_bounds__(256) hgx_hop_init(HopArgs a, int32_t n_pairs) {
    const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const int32_t h = a.hops[p];
    if (h >= 0) a.key[a.off[p] + h] = ((u64)(uint32_t)a.goal[p] << 32) | 0xFFFFFFFFull;
}

// Step k of the backtrace: one wavefront per (pair, slice).  The current node n sits at path position
// d = hops - k + 1 (the goal for k == 1, else what step k - 1 finished); its predecessor goes to position
// d - 1.  A row of at most kHeavyDegree entries is walked by slice 0 alone; a longer one by every slice,
// 64 entries at a time, strided by the slice count, so no wavefront walks a hub's row alone; the slices
// meet in the same atomicMin.
template <class M>
__global__ void __launch_bounds__(256) hgx_hop_step(HopArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    if (wave >= a.n_list) return;   // wave-uniform (as every return below)
    const int32_t pair = a.list[wave];
    const int32_t h = a.hops[pair];
    if (h < a.k) return;
    const int32_t d = h - a.k + 1;
    const int64_t o = a.off[pair];
    const int32_t n = (int32_t)(a.key[o + d] >> 32);
    if (n < 0) return;   // a broken chain (never in a consistent result): the readers see the missing key
    const HopSeed s = a.seeds[a.pair_seed[pair]];
    int64_t b = a.g.inc_off[n];
    const int64_t e = a.g.inc_off[n + 1];
    int64_t stride = 64;
    if (e - b <= kHeavyDegree) {
        if (blockIdx.y != 0) return;
    } else {
        b += (int64_t)blockIdx.y * 64;
        stride = (int64_t)gridDim.y * 64;
    }
    Counts c;
    u64 best = kNoKey;
    for (int64_t e0 = b; e0 < e; e0 += stride) {
        const int64_t ei = e0 + lane;
        if (ei < e) {
            const u64 k = hop_entry(a.g, n, ei, c, [&](int32_t t) { return M::in_level(s, d - 1, t, c); });
            best = k < best ? k : best;
        }
    }
    // every lane of the wavefront is here (the returns above and the loop bounds are wave-uniform)
    best = wave_min(best);
    if (lane == 0 && best != kNoKey) atomicMin(a.key + o + d - 1, best);
    wave_count(a.ctr, c, lane);
}

// One lane per pair: keys -> atoms (start .. goal) and links.
__global__ void __launch_bounds__(256) hgx_hop_write(HopArgs a, int32_t n_pairs, int32_t* __restrict__ atoms,
                                                      int32_t* __restrict__ links) {
    const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const int32_t h = a.hops[p];
    if (h < 0) return;
    const int64_t o = a.off[p], lo = a.loff[p];
    for (int32_t j = 0; j <= h; ++j) {
        const u64 k = a.key[o + j];
        atoms[o + j] = (int32_t)(k >> 32);
        if (j < h) links[lo + j] = (int32_t)(uint32_t)k;
    }
}

// depth[a] = the level of atom a for one seed (-1: not reached).
template <class M>
__global__ void __launch_bounds__(256) hgx_hop_depth_row(int64_t A, HopSeed s, int32_t* __restrict__ depth) {
    Counts c;
    for (int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; a < A; a += (int64_t)gridDim.x * blockDim.x)
        depth[a] = M::depth_of(s, (int32_t)a, c);
}

// key[n] of every atom for one seed: a group of 8 lanes per atom with at most kHeavyDegree entries (its lanes
// stride over the entries); kNoKey for the seed, the unreached atoms and, until hgx_hop_pred_heavy ran, the
// atoms with longer rows.
__global__ void __launch_bounds__(256) hgx_hop_pred_row(HopGraph g, const int32_t* __restrict__ depth, u64* __restrict__ key) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    Counts c;
    for (int64_t base = wave * 8; base < g.A; base += nwaves * 8) {   // wave-uniform
        const int64_t n = base + (lane >> 3);
        int64_t b = 0, e = 0;
        int32_t dn = -1;
        if (n < g.A) {
            dn = depth[n];
            if (dn >= 1) {
                b = g.inc_off[n];
                e = g.inc_off[n + 1];
                if (e - b > kHeavyDegree) e = b;
            }
        }
        u64 best = kNoKey;
        for (int64_t ei = b + (lane & 7); ei < e; ei += 8) {
            const u64 k = hop_entry(g, (int32_t)n, ei, c, [&](int32_t t) { return depth[t] == dn - 1; });
            best = k < best ? k : best;
        }
        // every lane of the wavefront is here again: the group's minimum
        for (int o = 4; o > 0; o >>= 1) {
            const u64 w = __shfl_xor(best, o, 64);
            best = w < best ? w : best;
        }
        if (n < g.A && (lane & 7) == 0) key[n] = best;
    }
}

// The atoms with more than kHeavyDegree entries, chunk by chunk of the snapshot's heavy-chunk table: one
// workgroup per chunk, a wavefront minimum and one atomicMin per wavefront.
__global__ void __launch_bounds__(256) hgx_hop_pred_heavy(HopGraph g, const HeavyChunk* __restrict__ chunks, int64_t n_chunks,
                                                           const int32_t* __restrict__ depth, u64* __restrict__ key) {
    const int lane = threadIdx.x & 63;
    Counts c;
    for (int64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {   // block-uniform
        const HeavyChunk k = chunks[ch];
        const int32_t n = k.atom;
        const int32_t dn = depth[n];
        if (dn < 1) continue;
        u64 best = kNoKey;
        for (int64_t e0 = k.beg + (threadIdx.x & ~63); e0 < k.end; e0 += blockDim.x) {
            const int64_t ei = e0 + lane;
            if (ei < k.end) {
                const u64 v = hop_entry(g, n, ei, c, [&](int32_t t) { return depth[t] == dn - 1; });
                best = v < best ? v : best;
            }
        }
        best = wave_min(best);   // wave-uniform: the loop bounds depend on the wavefront only
        if (lane == 0 && best != kNoKey) atomicMin(key + n, best);
    }
}

// Pool buffers of one call, handed back when it ends (after the stream drained: kernels may still read them
// on an error path).
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

HopGraph graph_args(const hgx_bfs_result* r) {
    const hgx_graph* g = r->g;
    HopGraph a{};
    a.A = g->A;
    a.mode = mode_of(r->opts);
    a.want_type = r->opts.link_type >= 0 ? r->opts.link_type : -1;
    a.inc_off = g->inc_off;
    a.inc_row = g->inc_row;
    a.inc_type = r->pred ? r->pred->inc_flag : g->inc_type;   // (want_type is then the predicate key)
    a.tgt_off = g->tgt_off;
    a.tgt_idx = g->tgt_idx;
    a.link_atom = g->link_atom;
    return a;
}

// The membership data of the distinct seeds a call asks for: host descriptors first (offsets into the two
// staging vectors), device pointers once both are uploaded.
struct SeedSet {
    std::vector<HopSeed> desc;
    std::vector<char> is_table;
    std::vector<int64_t> ptr_off, tab_off;     // per seed: offset into ptrs / tabs (-1: the other kind)
    std::vector<const void*> ptrs;             // per batch in use: fa[0 .. nlev), lvl[0 .. nlev)
    std::vector<u64> tabs;
    std::unordered_map<int32_t, int64_t> batch_off;

    // Caller holds g->mu with g's device current.
    int32_t add(hgx_bfs_result* r, int32_t si) {
        hgx_graph* g = r->g;
        HopSeed s{};
        int64_t po = -1, to = -1;
        if (r->blk && r->blk->pairs[si] >= 0) {   // a workgroup / grid-stage seed: its sorted (atom, depth) table
            block_materialize(g, *r->blk);
            const BlockSet& b = *r->blk;
            to = (int64_t)tabs.size();
            tabs.push_back((u64)(uint32_t)b.seeds[si] << 32);
            int64_t k = 0;
            for (int32_t d = 0; d < b.levels[si]; ++d)
                for (int64_t e = k + b.lcnt[si][d]; k < e; ++k)
                    tabs.push_back(((u64)(uint32_t)b.atoms[si][k] << 32) | (u64)(uint32_t)(d + 1));
            std::sort(tabs.begin() + to, tabs.end());
            s.n_tab = (int32_t)((int64_t)tabs.size() - to);
        } else {
            const int32_t ci = r->blk ? r->compact[si] : si;
            const int32_t bi = ci / 1024;
            const BfsBatch& bt = r->batches[bi];
            const int32_t nl = (int32_t)bt.lvl.size();
            auto it = batch_off.find(bi);
            if (it == batch_off.end()) {
                po = (int64_t)ptrs.size();
                for (int32_t k = 0; k < nl; ++k) ptrs.push_back(bt.fa[k]);
                for (int32_t k = 0; k < nl; ++k) ptrs.push_back(bt.lvl[k]);
                batch_off.emplace(bi, po);
            } else {
                po = it->second;
            }
            s.nlev = nl;
            s.W = bt.W;
            s.bit = ci % 1024;
        }
        desc.push_back(s);
        is_table.push_back(to >= 0);
        ptr_off.push_back(po);
        tab_off.push_back(to);
        return (int32_t)desc.size() - 1;
    }
    void resolve(Scratch& sc) {
        const void** dp = sc.upload(ptrs);
        const u64* dt = sc.upload(tabs);
        for (size_t i = 0; i < desc.size(); ++i) {
            if (is_table[i]) {
                desc[i].tab = dt + tab_off[i];
            } else {
                desc[i].fa = (const u64* const*)(dp + ptr_off[i]);
                desc[i].lvl = (const u64* const*)(dp + ptr_off[i] + desc[i].nlev);
            }
        }
    }
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

// The depth row (and, with need_key, the predecessor-key row) of seed si, cached on the result.  Caller holds
// g->mu with g's device current.
void ensure_rows(hgx_bfs_result* r, int32_t si, bool need_key) {
    hgx_graph* g = r->g;
    const int64_t A = g->A;
    const size_t n = (size_t)std::max<int64_t>(A, 1);
    hipStream_t st = g->stream;
    if (!r->hop_depth) r->hop_depth = (int32_t*)g->alloc(sizeof(int32_t) * n);
    if (r->hop_seed != si) {
        r->hop_seed = -1;
        r->hop_have_key = false;
        Scratch sc(g);
        SeedSet ss;
        ss.add(r, si);
        ss.resolve(sc);
        if (A > 0) {
            const int grid = grid_for(A, 256, 4096);
            if (ss.is_table[0]) hgx_hop_depth_row<TableMember><<<grid, 256, 0, st>>>(A, ss.desc[0], r->hop_depth);
            else hgx_hop_depth_row<RowsMember><<<grid, 256, 0, st>>>(A, ss.desc[0], r->hop_depth);
            HGX_CHECK_LAUNCH();
        }
        HGX_HIP(hipStreamSynchronize(st));
        r->hop_seed = si;
    }
    if (need_key && !r->hop_have_key) {
        if (!r->hop_key) r->hop_key = (u64*)g->alloc(sizeof(u64) * n);
        if (A > 0) {
            const HopGraph ga = graph_args(r);
            hgx_hop_pred_row<<<grid_for(A * 8, 256, 8192), 256, 0, st>>>(ga, r->hop_depth, r->hop_key);
            HGX_CHECK_LAUNCH();
            if (g->n_chunks > 0) {
                hgx_hop_pred_heavy<<<(int)std::min<int64_t>(g->n_chunks, 8192), 256, 0, st>>>(ga, g->chunks, g->n_chunks,
                                                                                              r->hop_depth, r->hop_key);
                HGX_CHECK_LAUNCH();
            }
        }
        HGX_HIP(hipStreamSynchronize(st));
        r->hop_have_key = true;
    }
}

void check_row_args(const char* fn, const hgx_bfs_result* r, int32_t seed_index, int64_t first, int64_t n, bool outs) {
    if (!r || !outs || first < 0 || n < 0) fail(HGX_E_INVALID, std::string(fn) + ": bad argument");
    if (r->g->shard) fail(HGX_E_UNSUPPORTED, std::string(fn) + ": the result of a partition shard holds owned atoms only");
    if (seed_index < 0 || seed_index >= r->n_seeds) fail(HGX_E_NOTFOUND, std::string(fn) + ": no such seed index");
    if (first + n > r->g->A) fail(HGX_E_INVALID, std::string(fn) + ": atom range out of bounds");
}

}  // namespace
}  // namespace hgx

using namespace hgx;

struct hgx_hop_paths {
    int32_t n_pairs = 0;
    int64_t total_atoms = 0, n_reached = 0;
    std::vector<int32_t> hops;
    std::vector<int64_t> off;      // [n_pairs + 1]
    std::vector<int32_t> atoms, links;
    int64_t steps = 0, entries = 0, pins = 0, fa_probes = 0, row_probes = 0;
    double ms_total = 0, bytes = 0;
};

extern "C" {

int hgx_bfs_result_paths(hgx_bfs_result* r, const int32_t* seed_index, const int32_t* goal, int32_t n_pairs,
                         hgx_hop_paths** out) {
    HGX_API_BEGIN
    if (!r || !out || n_pairs < 0 || (n_pairs > 0 && (!seed_index || !goal)))
        fail(HGX_E_INVALID, "hgx_bfs_result_paths: bad argument");
    hgx_graph* g = r->g;
    if (g->shard) fail(HGX_E_UNSUPPORTED, "hgx_bfs_result_paths: the result of a partition shard holds owned atoms only");
    for (int32_t i = 0; i < n_pairs; ++i) {
        if (seed_index[i] < 0 || seed_index[i] >= r->n_seeds)
            fail(HGX_E_NOTFOUND, "hgx_bfs_result_paths: pair " + std::to_string(i) + ": no such seed index " +
                                     std::to_string(seed_index[i]));
        if (goal[i] < 0 || goal[i] >= g->A)
            fail(HGX_E_INVALID, "hgx_bfs_result_paths: pair " + std::to_string(i) + ": goal " + std::to_string(goal[i]) +
                                    " out of range");
    }
    std::unique_ptr<hgx_hop_paths> p(new hgx_hop_paths());
    p->n_pairs = n_pairs;
    p->hops.assign((size_t)n_pairs, -1);
    p->off.assign((size_t)n_pairs + 1, 0);
    if (n_pairs == 0) {
        *out = p.release();
        return HGX_OK;
    }
    std::lock_guard<std::mutex> lk(g->mu);
    HGX_HIP(hipSetDevice(g->device));
    hipStream_t st = g->stream;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    struct EvGuard {   // timing events go back to the graph's pool (g->mu is held)
        hgx_graph* g;
        hipEvent_t* ev;
        ~EvGuard() {
            for (int i = 0; i < 4; ++i)
                if (ev[i]) g->ev_pool.push_back(ev[i]);
        }
    } evg{g, ev};
    if (g->timing)
        for (auto& e : ev) e = take_event(g);
    Scratch sc(g);

    // the distinct requested seeds and the pairs of each membership kind
    SeedSet ss;
    std::unordered_map<int32_t, int32_t> seen;
    std::vector<int32_t> pair_seed((size_t)n_pairs), list[2];
    for (int32_t i = 0; i < n_pairs; ++i) {
        auto it = seen.find(seed_index[i]);
        if (it == seen.end()) it = seen.emplace(seed_index[i], ss.add(r, seed_index[i])).first;
        pair_seed[(size_t)i] = it->second;
        list[ss.is_table[(size_t)it->second] ? 1 : 0].push_back(i);
    }
    ss.resolve(sc);

    HopArgs a{};
    a.g = graph_args(r);
    a.seeds = sc.upload(ss.desc);
    a.pair_seed = sc.upload(pair_seed);
    {
        std::vector<int32_t> hg(goal, goal + n_pairs);
        a.goal = sc.upload(hg);
        HGX_HIP(hipStreamSynchronize(st));   // hg leaves scope
    }
    a.hops = sc.get<int32_t>((size_t)n_pairs);
    a.ctr = sc.get<u64>(cWords);
    const int32_t* dlist[2] = {sc.upload(list[0]), sc.upload(list[1])};
    HGX_HIP(hipMemsetAsync(a.ctr, 0, sizeof(u64) * cWords, st));

    if (ev[0]) HGX_HIP(hipEventRecord(ev[0], st));
    for (int kind = 0; kind < 2; ++kind) {
        if (list[kind].empty()) continue;
        a.list = dlist[kind];
        a.n_list = (int32_t)list[kind].size();
        const int grid = (int)ceil_div(a.n_list, 4);
        if (kind == 0) hgx_hop_depth<RowsMember><<<grid, 256, 0, st>>>(a);
        else hgx_hop_depth<TableMember><<<grid, 256, 0, st>>>(a);
        HGX_CHECK_LAUNCH();
    }
    HGX_HIP(hipMemcpyAsync(p->hops.data(), a.hops, sizeof(int32_t) * (size_t)n_pairs, hipMemcpyDeviceToHost, st));
    if (ev[1]) HGX_HIP(hipEventRecord(ev[1], st));
    HGX_HIP(hipStreamSynchronize(st));

    std::vector<int64_t> loff((size_t)n_pairs);
    int32_t max_hops[2] = {0, 0};
    int64_t total = 0, reached = 0;
    for (int32_t i = 0; i < n_pairs; ++i) {
        p->off[(size_t)i] = total;
        loff[(size_t)i] = total - reached;
        const int32_t h = p->hops[(size_t)i];
        if (h >= 0) {
            total += (int64_t)h + 1;
            ++reached;
            int32_t& m = max_hops[ss.is_table[(size_t)pair_seed[(size_t)i]] ? 1 : 0];
            m = std::max(m, h);
        }
    }
    p->off[(size_t)n_pairs] = total;
    p->total_atoms = total;
    p->n_reached = reached;
    p->atoms.assign((size_t)total, -1);
    p->links.assign((size_t)(total - reached), -1);

    if (total > 0) {
        a.off = sc.upload(p->off);
        a.loff = sc.upload(loff);
        a.key = sc.get<u64>((size_t)total);
        int32_t* datoms = sc.get<int32_t>((size_t)total);
        int32_t* dlinks = sc.get<int32_t>((size_t)(total - reached));
        if (ev[2]) HGX_HIP(hipEventRecord(ev[2], st));
        HGX_HIP(hipMemsetAsync(a.key, 0xFF, sizeof(u64) * (size_t)total, st));
        hgx_hop_init<<<(int)ceil_div(n_pairs, 256), 256, 0, st>>>(a, n_pairs);
        HGX_CHECK_LAUNCH();
        // the slices of a step: enough that one of them takes about kChunkEntries entries of the longest row
        const int slices = (int)std::min<int64_t>(std::max<int64_t>(g->n_chunks, 1), 128);
        for (int32_t k = 1; k <= std::max(max_hops[0], max_hops[1]); ++k) {
            a.k = k;
            for (int kind = 0; kind < 2; ++kind) {
                if (list[kind].empty() || max_hops[kind] < k) continue;
                a.list = dlist[kind];
                a.n_list = (int32_t)list[kind].size();
                const dim3 grid((unsigned)ceil_div(a.n_list, 4), (unsigned)slices);
                if (kind == 0) hgx_hop_step<RowsMember><<<grid, 256, 0, st>>>(a);
                else hgx_hop_step<TableMember><<<grid, 256, 0, st>>>(a);
                HGX_CHECK_LAUNCH();
                ++p->steps;
            }
        }
        hgx_hop_write<<<(int)ceil_div(n_pairs, 256), 256, 0, st>>>(a, n_pairs, datoms, dlinks);
        HGX_CHECK_LAUNCH();
        HGX_HIP(hipMemcpyAsync(p->atoms.data(), datoms, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, st));
        if (total > reached)
            HGX_HIP(hipMemcpyAsync(p->links.data(), dlinks, sizeof(int32_t) * (size_t)(total - reached),
                                   hipMemcpyDeviceToHost, st));
        if (ev[3]) HGX_HIP(hipEventRecord(ev[3], st));
    }
    u64 hc[cWords] = {};
    HGX_HIP(hipMemcpyAsync(hc, a.ctr, sizeof(hc), hipMemcpyDeviceToHost, st));
    HGX_HIP(hipStreamSynchronize(st));
    for (int64_t i = 0; i < total; ++i)
        if (p->atoms[(size_t)i] < 0) fail(HGX_E_DEVICE, "hgx_bfs_result_paths: a path atom has no predecessor in the level before it");
    p->entries = (int64_t)hc[cEntries];
    p->pins = (int64_t)hc[cPins];
    p->fa_probes = (int64_t)hc[cFaProbes];
    p->row_probes = (int64_t)hc[cRowProbes];
    // algorithmic bytes: per entry the row id, the type (typed) and the two target offsets,
    // per pin 4, per probe the fa word and, behind a set bit, the row word (a table probe: 8 per search step)
    p->bytes = (double)p->entries * (4.0 + (a.g.want_type >= 0 ? 4.0 : 0.0) + 16.0) + 4.0 * (double)p->pins +
               8.0 * (double)p->fa_probes + 8.0 * (double)p->row_probes;
    if (ev[0]) {
        float ms = 0;
        HGX_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        p->ms_total = ms;
        if (total > 0) {
            HGX_HIP(hipEventElapsedTime(&ms, ev[2], ev[3]));
            p->ms_total += ms;
        }
    }
    *out = p.release();
    HGX_API_END
}

int hgx_hop_paths_info(const hgx_hop_paths* p, int32_t* n_pairs, int64_t* total_atoms) {
    HGX_API_BEGIN
    if (!p) fail(HGX_E_INVALID, "hgx_hop_paths_info: null result");
    if (n_pairs) *n_pairs = p->n_pairs;
    if (total_atoms) *total_atoms = p->total_atoms;
    HGX_API_END
}

int hgx_hop_paths_offsets(const hgx_hop_paths* p, int64_t* off, int32_t* hops) {
    HGX_API_BEGIN
    if (!p) fail(HGX_E_INVALID, "hgx_hop_paths_offsets: null result");
    if (off) std::memcpy(off, p->off.data(), sizeof(int64_t) * p->off.size());
    if (hops && p->n_pairs) std::memcpy(hops, p->hops.data(), sizeof(int32_t) * p->hops.size());
    HGX_API_END
}

int hgx_hop_paths_read(const hgx_hop_paths* p, int32_t* atoms, int32_t* links) {
    HGX_API_BEGIN
    if (!p) fail(HGX_E_INVALID, "hgx_hop_paths_read: null result");
    if (atoms && !p->atoms.empty()) std::memcpy(atoms, p->atoms.data(), sizeof(int32_t) * p->atoms.size());
    if (links && !p->links.empty()) std::memcpy(links, p->links.data(), sizeof(int32_t) * p->links.size());
    HGX_API_END
}

int hgx_hop_paths_stats(const hgx_hop_paths* p, int64_t* steps, int64_t* entries, int64_t* probes, double* ms_total,
                        double* bytes) {
    HGX_API_BEGIN
    if (!p) fail(HGX_E_INVALID, "hgx_hop_paths_stats: null result");
    if (steps) *steps = p->steps;
    if (entries) *entries = p->entries;
    if (probes) *probes = p->fa_probes;
    if (ms_total) *ms_total = p->ms_total;
    if (bytes) *bytes = p->bytes;
    HGX_API_END
}

void hgx_hop_paths_free(hgx_hop_paths* p) { delete p; }

int hgx_bfs_result_depth_row(hgx_bfs_result* r, int32_t seed_index, int64_t first, int64_t n, int32_t* depth) {
    HGX_API_BEGIN
    check_row_args("hgx_bfs_result_depth_row", r, seed_index, first, n, depth != nullptr || n == 0);
    if (n == 0) return HGX_OK;
    hgx_graph* g = r->g;
    std::lock_guard<std::mutex> lk(g->mu);
    HGX_HIP(hipSetDevice(g->device));
    ensure_rows(r, seed_index, false);
    HGX_HIP(hipMemcpyAsync(depth, r->hop_depth + first, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, g->stream));
    HGX_HIP(hipStreamSynchronize(g->stream));
    HGX_API_END
}

int hgx_bfs_result_predecessor_row(hgx_bfs_result* r, int32_t seed_index, int64_t first, int64_t n, int32_t* pred_atom,
                                   int32_t* pred_link) {
    HGX_API_BEGIN
    check_row_args("hgx_bfs_result_predecessor_row", r, seed_index, first, n, (pred_atom && pred_link) || n == 0);
    if (n == 0) return HGX_OK;
    hgx_graph* g = r->g;
    std::lock_guard<std::mutex> lk(g->mu);
    HGX_HIP(hipSetDevice(g->device));
    ensure_rows(r, seed_index, true);
    std::vector<u64> k((size_t)n);
    HGX_HIP(hipMemcpyAsync(k.data(), r->hop_key + first, sizeof(u64) * (size_t)n, hipMemcpyDeviceToHost, g->stream));
    HGX_HIP(hipStreamSynchronize(g->stream));
    for (int64_t i = 0; i < n; ++i) {   // the keys split into atom / link; kNoKey gives -1 / -1
        pred_atom[i] = (int32_t)(k[(size_t)i] >> 32);
        pred_link[i] = (int32_t)(uint32_t)k[(size_t)i];
    }
    HGX_API_END
}

}  // extern "C"
