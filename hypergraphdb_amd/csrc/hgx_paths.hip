// hgx_paths.hip -- batched weighted shortest paths (include/hgx_paths.h).
//
// Replaces GraphClassics.dijkstra (C/algorithms/GraphClassics.java:126-209) over a DefaultALGenerator
// (C/algorithms/DefaultALGenerator.java:73-593) for many (start, goal) pairs at once.  The reference's
// formulation is serial (a TreeSet ordered by tentative distance); its RESULT is the least fixed point
// of the min-plus relaxation  d(n) = min over edges a -> n of d(a) + w,  d(start) = 0,  and for finite
// weights >= 0 that fixed point does not depend on the order of relaxation, bit for bit.
// So the engine is label-correcting:
//
//   dist[pair][atom] : the bit pattern of a non-negative double (orders as an unsigned integer),
//                      lowered with a 64-bit atomicMin
//   frontier         : (pair, atom[, chunk]) items whose distance was lowered in the previous round
//   round            : one launch; a wavefront takes an item, walks the atom's incidence entries (a
//                      lane per entry) with the generator's position rule and relaxes every yielded
//                      target; an atom that improved is queued once per round (a round stamp)
//
// and it stops when a round queues nothing.  Goal pairs skip atoms that are no nearer than the goal.
// After convergence the predecessors (rule R of hgx_paths.h) come from sweeps over the atoms with a
// final distance, and one lane per goal pair walks them back from the goal.
//
// Edges: the closed-form neighbour rule of the set-mode BFS (hgx_bfs.hip mode_of; pyref.reachable): in
// a link with targets T, atom v at first / last position fv / lv yields the targets at the positions
//   symmetric: all;  after-first: > fv;  before-first: < fv;  before-last: < lv;  after-last: > lv
// other than v itself (a self-yield can lower nothing).  minArity only excludes links that yield nothing
// but the source.

#include <cmath>
#include <cstring>
#include <memory>

#include "hgx_internal.h"

namespace hgx {
namespace {

typedef unsigned long long u64;

constexpr u64 kInfBits = 0x7FF0000000000000ull;   // +inf: not reached
constexpr u64 kNone = ~0ull;                      // no predecessor key
constexpr uint32_t kNoLvl = 0xFFFFFFFFu;
// A frontier item: pair (20 bits) | chunk of a heavy atom's incidence (12 bits) | atom (32 bits).
constexpr int kPairShift = 44, kSubShift = 32;
constexpr int64_t kMaxChunkPairs = (int64_t)1 << 20;
constexpr int64_t kMaxSubs = 4096;

// Device words of one call: two frontier counters, then the statistics and flags.
enum { cCnt0 = 0, cCnt1 = 1, cExpanded = 2, cEntries = 3, cRelaxed = 4, cImproved = 5, cOverflow = 6, cChanged = 7,
       cPlateau = 8, cWords = 16 };

struct SpArgs {
    int64_t A;
    int64_t K;                 // pairs of this chunk
    int32_t mode, want_type;
    const int64_t* inc_off;
    const int32_t* inc_row;
    const int32_t* inc_type;
    const int64_t* tgt_off;
    const int32_t* tgt_idx;
    const int32_t* link_atom;
    const double* w;           // per link row; nullptr = 1.0
    const int32_t* starts;     // [K]
    const int32_t* goals;      // [K]
    u64* dist;                 // [K * A]
    uint32_t* stamp;           // [K * A] round an atom was last queued in; after convergence: plateau levels
    u64* pd;                   // [K * A] least distance of a tight predecessor
    u64* pk;                   // [K * A] (predecessor atom << 32) | link atom
    const u64* keep;           // sibling predicate: bit t set = atom t may be yielded; nullptr = no test
    const u64* items;          // this launch's work items
    int64_t n_items;
    u64* next;                 // the list this launch appends to, its counter and capacity
    u64* next_cnt;
    int64_t cap;
    u64* ctr;                  // the call's device words (c* above)
    uint32_t round;
    int32_t use_lvl;
};

__device__ __forceinline__ u64 ld64(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t ld32(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double as_double(u64 b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ u64 as_bits(double d) { return (u64)__double_as_longlong(d); }

// Incidence rows above kHeavyDegree are walked in chunks of at least kChunkEntries entries, at most
// kMaxSubs of them (one work item each), so one wavefront never walks a million-entry row alone.
__host__ __device__ __forceinline__ int64_t sp_chunk(int64_t deg) {
    const int64_t need = (deg + kMaxSubs - 1) / kMaxSubs;
    return need > kChunkEntries ? need : kChunkEntries;
}
__host__ __device__ __forceinline__ int64_t sp_subs(int64_t deg) {
    if (deg <= kHeavyDegree) return 1;
    const int64_t c = sp_chunk(deg);
    return (deg + c - 1) / c;
}
__device__ __forceinline__ u64 sp_item(int64_t pair, int64_t sub, int32_t atom) {
    return ((u64)pair << kPairShift) | ((u64)sub << kSubShift) | (u64)(uint32_t)atom;
}

// Appends the work items of atom t of `pair` (want lanes only) to a.next.  Called by every lane of the
// wavefront together: the light atoms' items take one counter atomic per wavefront (ballot + popcount),
// a heavy atom's chunk items one atomic of their own.  Atoms without incidence have nothing to expand.
__device__ __forceinline__ void sp_append(const SpArgs& a, bool want, int64_t pair, int32_t t) {
    int64_t deg = 0;
    if (want) deg = a.inc_off[t + 1] - a.inc_off[t];
    const bool heavy = want && deg > kHeavyDegree;
    const bool light = want && deg > 0 && !heavy;
    const u64 m = __ballot(light);
    if (m) {
        const int lane = threadIdx.x & 63;
        const int leader = __ffsll((long long)m) - 1;
        u64 base = 0;
        if (lane == leader) base = atomicAdd(a.next_cnt, (u64)__popcll(m));
        base = __shfl(base, leader);
        if (light) {
            const int64_t pos = (int64_t)base + __popcll(m & ((1ull << lane) - 1ull));
            if (pos < a.cap) a.next[pos] = sp_item(pair, 0, t);
            else atomicOr(a.ctr + cOverflow, 1ull);
        }
    }
    if (heavy) {
        const int64_t ns = sp_subs(deg);
        const int64_t base = (int64_t)atomicAdd(a.next_cnt, (u64)ns);
        for (int64_t s = 0; s < ns; ++s) {
            if (base + s < a.cap) a.next[base + s] = sp_item(pair, s, t);
            else atomicOr(a.ctr + cOverflow, 1ull);
        }
    }
}

// dist = +inf over the chunk.
__global__ void __launch_bounds__(256) hgx_sp_fill(int64_t n, u64* __restrict__ dist) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dist[i] = kInfBits;
}

// dm.put(start, 0.0); unsettled.add(start) (GraphClassics.java:135,172), one wavefront-wide pass per 64 pairs.
__global__ void __launch_bounds__(64) hgx_sp_seed(SpArgs a) {
    const int64_t p = blockIdx.x * (int64_t)64 + threadIdx.x;
    bool want = false;
    int32_t s = 0;
    if (p < a.K) {
        s = a.starts[p];
        a.dist[p * a.A + s] = 0ull;
        want = s != a.goals[p];   // start == goal: distance 0, nothing to expand
    }
    sp_append(a, want, p, s);
}

enum { kRelax = 0, kPredDist = 1, kLevels = 2, kPredKey = 3 };

// One wavefront per work item.  OP:
//   kRelax    the relaxation round (GraphClassics.java:180-205 for every queued atom at once)
//   kPredDist pd[n] = min d(a) over the tight edges a -> n (d(a) + w == d(n))
//   kLevels   plateau levels: along tight edges with d(a) == d(n), lvl[n] = min(lvl[a] + 1)
//   kPredKey  pk[n] = min (a << 32 | link atom) over the tight edges with d(a) == pd[n]
template <int OP>
__global__ void __launch_bounds__(256) hgx_sp_walk(SpArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    u64 c_exp = 0, c_ent = 0, c_rel = 0, c_imp = 0;   // wavefront-uniform
    bool changed = false;
    for (int64_t it = wave; it < a.n_items; it += nwaves) {
        const u64 item = a.items[it];
        const int64_t pair = (int64_t)(item >> kPairShift);
        const int64_t sub = (int64_t)((item >> kSubShift) & (u64)(kMaxSubs - 1));
        const int32_t v = (int32_t)(uint32_t)item;
        const int64_t base = pair * a.A;
        const int32_t start = a.starts[pair], goal = a.goals[pair];
        const u64 dv = ld64(a.dist + base + v);
        const u64 dg = goal >= 0 ? ld64(a.dist + base + goal) : kInfBits;
        if (OP == kRelax && dv >= dg) continue;   // no nearer than the goal: its edges cannot matter
        uint32_t lv_v = 0;
        if (OP == kLevels || (OP == kPredKey && a.use_lvl)) lv_v = ld32(a.stamp + base + v);
        if (OP == kLevels && lv_v == kNoLvl) continue;
        int64_t b = a.inc_off[v], e = a.inc_off[v + 1];
        if (e - b > kHeavyDegree) {
            const int64_t ch = sp_chunk(e - b);
            b += sub * ch;
            e = b + ch < e ? b + ch : e;
        }
        ++c_exp;
        for (int64_t e0 = b; e0 < e; e0 += 64) {
            const int64_t ei = e0 + lane;
            int64_t p = 0, pe = 0;
            int32_t row = 0;
            u64 nd = 0;
            if (ei < e) {
                row = a.inc_row[ei];
                if (a.want_type < 0 || a.inc_type[ei] == a.want_type) {   // linkPredicate (DefaultALGenerator.java:300-308)
                    p = a.tgt_off[row];
                    pe = a.tgt_off[row + 1];
                    if (a.mode != kSym) {
                        int64_t fv = -1, lv = -1;
                        for (int64_t q = p; q < pe; ++q)
                            if (a.tgt_idx[q] == v) {
                                if (fv < 0) fv = q;
                                lv = q;
                            }
                        if (a.mode == kAfterFirst) p = fv + 1;
                        else if (a.mode == kBeforeFirst) pe = fv;
                        else if (a.mode == kBeforeLast) pe = lv;
                        else p = lv + 1;
                    }
                    nd = as_bits(as_double(dv) + (a.w ? a.w[row] : 1.0));   // weightCurrent + weightAN (:191,196)
                }
            }
            c_ent += (u64)__popcll(__ballot(ei < e));
            while (__ballot(p < pe)) {
                bool act = p < pe;
                int32_t t = -1;
                if (act) {
                    t = a.tgt_idx[p];
                    ++p;
                    // (siblingPredicate: a target that fails is not yielded, DefaultALGenerator.java:120-150)
                    act = t != v && (!a.keep || ((a.keep[t >> 6] >> (t & 63)) & 1ull));
                }
                if (OP == kRelax) {
                    bool imp = false, app = false;
                    act = act && nd <= dg;   // past the goal: never expanded, never on its path
                    if (act) {
                        u64* dp = a.dist + base + t;
                        u64 old = ld64(dp);   // a stale (larger) value only costs the atomic
                        if (nd < old) {
                            old = atomicMin(dp, nd);
                            imp = nd < old;
                        }
                        if (imp) app = atomicExch(a.stamp + base + t, a.round) != a.round;
                    }
                    c_rel += (u64)__popcll(__ballot(act));
                    c_imp += (u64)__popcll(__ballot(imp));
                    sp_append(a, app, pair, t);
                } else if (act && t != start) {
                    const u64 dt = a.dist[base + t];
                    if (dt != kInfBits && dt <= dg && nd == dt) {   // a tight edge inside the goal's radius
                        if (OP == kPredDist) {
                            atomicMin(a.pd + base + t, dv);
                        } else if (OP == kLevels) {
                            if (dv == dt && a.pd[base + t] == dt) {
                                const uint32_t old = atomicMin(a.stamp + base + t, lv_v + 1u);
                                changed |= lv_v + 1u < old;
                            }
                        } else if (a.pd[base + t] == dv) {
                            bool ok = true;
                            if (a.use_lvl && dv == dt) ok = lv_v != kNoLvl && lv_v + 1u == a.stamp[base + t];
                            if (ok)
                                atomicMin(a.pk + base + t, ((u64)(uint32_t)v << 32) | (u64)(uint32_t)a.link_atom[row]);
                        }
                    }
                }
            }
        }
    }
    if (OP == kRelax && lane == 0 && c_exp) {
        atomicAdd(a.ctr + cExpanded, c_exp);
        atomicAdd(a.ctr + cEntries, c_ent);
        atomicAdd(a.ctr + cRelaxed, c_rel);
        atomicAdd(a.ctr + cImproved, c_imp);
    }
    if (OP == kLevels && changed) atomicOr(a.ctr + cChanged, 1ull);
}

// The work items of the predecessor sweeps: every (pair, atom) with a final distance inside the goal's
// radius (every reached atom of an HGX_NO_GOAL pair); nothing for start == goal or an unreached goal.
__global__ void __launch_bounds__(256) hgx_sp_reached(SpArgs a) {
    const int64_t total = a.K * a.A;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + (threadIdx.x & ~63); i0 < total; i0 += stride) {
        const int64_t i = i0 + (threadIdx.x & 63);
        bool want = false;
        int64_t pair = 0;
        int32_t v = 0;
        if (i < total) {
            pair = i / a.A;
            v = (int32_t)(i - pair * a.A);
            const int32_t start = a.starts[pair], goal = a.goals[pair];
            const u64 d = a.dist[i];
            const u64 dg = goal >= 0 ? a.dist[pair * a.A + goal] : kInfBits;
            want = start != goal && d != kInfBits && (goal < 0 || (dg != kInfBits && d <= dg));
        }
        sp_append(a, want, pair, v);
    }
}

// Plateau levels start: 0 for the start and for every atom with a strictly nearer tight predecessor,
// none for the others; counts the atoms whose nearest tight predecessor is exactly as far as they are
// (zero or absorbed weights -- none when every relaxation was strictly inflationary).
__global__ void __launch_bounds__(256) hgx_sp_plateau(SpArgs a) {
    const int64_t total = a.K * a.A;
    u64 n = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pair = i / a.A;
        const int32_t v = (int32_t)(i - pair * a.A);
        const u64 p = a.pd[i], d = a.dist[i];
        uint32_t l = kNoLvl;
        if (p == kNone) l = v == a.starts[pair] ? 0u : kNoLvl;
        else if (p < d) l = 0u;
        else ++n;
        a.stamp[i] = l;
    }
    if (n) atomicAdd(a.ctr + cPlateau, n);
}

// Per pair: the goal's distance and the number of atoms on its path (0: none, -1: broken chain).
__global__ void __launch_bounds__(64) hgx_sp_path_len(SpArgs a, u64* __restrict__ gdist, int64_t* __restrict__ len) {
    const int64_t p = blockIdx.x * (int64_t)64 + threadIdx.x;
    if (p >= a.K) return;
    const int32_t start = a.starts[p], goal = a.goals[p];
    const int64_t base = p * a.A;
    if (goal < 0) {
        gdist[p] = 0ull;
        len[p] = 0;
        return;
    }
    const u64 dg = a.dist[base + goal];
    gdist[p] = dg;
    int64_t c = 0;
    if (dg != kInfBits) {
        c = 1;
        int32_t n = goal;
        while (n != start) {
            const u64 k = a.pk[base + n];
            if (k == kNone || c > a.A) {
                c = -1;
                break;
            }
            n = (int32_t)(k >> 32);
            ++c;
        }
    }
    len[p] = c;
}

// atoms[off[p], off[p + 1]) = start .. goal; links[off[p] + k] joins atoms k - 1 and k (slot 0 unused).
__global__ void __launch_bounds__(64) hgx_sp_path_write(SpArgs a, const int64_t* __restrict__ off, int32_t* __restrict__ atoms,
                                                         int32_t* __restrict__ links) {
    const int64_t p = blockIdx.x * (int64_t)64 + threadIdx.x;
    if (p >= a.K) return;
    const int64_t o = off[p], L = off[p + 1] - o;
    if (L <= 0) return;
    const int64_t base = p * a.A;
    int32_t n = a.goals[p];
    int64_t i = L - 1;
    atoms[o + i] = n;
    while (i > 0) {
        const u64 k = a.pk[base + n];
        links[o + i] = (int32_t)(uint32_t)k;
        n = (int32_t)(k >> 32);
        --i;
        atoms[o + i] = n;
    }
    links[o] = -1;
}

}  // namespace
}  // namespace hgx

using namespace hgx;

struct hgx_link_weights {
    int device = 0;
    int64_t M = 0;
    double* w = nullptr;   // [M] device
};

struct hgx_sp_result {
    hgx_graph* g = nullptr;
    hgx_link_predicate* pred = nullptr;   // the link predicate it was made with: a reference, kept for the lifetime rule
                                          // only (include/hgx_linkpred.h); no reader of this result uses it
    hgx_atom_predicate* apred = nullptr;  // its sibling predicate, likewise (include/hgx_sibling.h)
    int32_t n_pairs = 0;
    int64_t A = 0;
    std::vector<int32_t> goals;
    std::vector<double> dist;           // [n_pairs] d*(goal)
    std::vector<uint8_t> reached;
    std::vector<int64_t> path_off;      // [n_pairs + 1]
    std::vector<int32_t> path_atoms, path_links;   // links[path_off[i]] is unused
    struct Row {
        u64* dist = nullptr;   // [A] device (pool memory of g)
        u64* pk = nullptr;     // [A]
    };
    std::vector<Row> rows;              // [n_pairs], set for HGX_NO_GOAL pairs
    int64_t rounds = 0, expanded = 0, entries = 0, relaxed = 0, improved = 0;
    double ms_total = 0, bytes = 0;
};

namespace {

// Pool buffers of one call, handed back on every exit (the graph mutex is held throughout).
struct Scratch {
    hgx_graph* g;
    std::vector<PoolBuf> bufs;
    explicit Scratch(hgx_graph* g_) : g(g_) {}
    template <class T> T* get(int64_t n) {
        const size_t bytes = sizeof(T) * (size_t)std::max<int64_t>(n, 1);
        void* p = g->alloc(bytes);
        bufs.push_back({p, bytes});
        return (T*)p;
    }
    ~Scratch() {
        (void)hipStreamSynchronize(g->stream);
        for (auto& b : bufs) g->release(b.p, b.n);
    }
};

void release_rows(hgx_sp_result* r) {
    for (auto& row : r->rows) {
        if (row.dist) r->g->release(row.dist, sizeof(u64) * (size_t)r->A);
        if (row.pk) r->g->release(row.pk, sizeof(u64) * (size_t)r->A);
        row.dist = row.pk = nullptr;
    }
}

void sp_run(hgx_graph* g, const int32_t* starts, const int32_t* goals, int32_t n_pairs, const hgx_algen_opts& o,
            const hgx_link_weights* lw, hgx_sp_result* r) {
    hipStream_t s = g->stream;
    const int64_t A = g->A;
    // per pair: dist 8 + stamp 4 + predecessor keys 8 per atom, two item lists of A + (heavy chunks) entries
    const int64_t list_pp = A + g->n_chunks;
    const int64_t bytes_pp = 20 * A + 16 * list_pp;
    int64_t K = g->sp_budget_bytes / std::max<int64_t>(bytes_pp, 1);
    K = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(K, n_pairs), kMaxChunkPairs));

    Scratch sc(g);
    u64* dist = sc.get<u64>(K * A);
    uint32_t* stamp = sc.get<uint32_t>(K * A);
    u64* pk = sc.get<u64>(K * A);
    const int64_t cap = K * list_pp;
    u64* lists[2] = {sc.get<u64>(cap), sc.get<u64>(cap)};
    int32_t* d_sg = sc.get<int32_t>(2 * K);
    u64* ctr = sc.get<u64>(cWords);
    u64* d_gdist = sc.get<u64>(K);
    int64_t* d_len = sc.get<int64_t>(K + 1);
    u64* host = (u64*)g->pinned_buf(sizeof(u64) * cWords);

    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            for (int i = 0; i < 2; ++i)
                if (e[i]) (void)hipEventDestroy(e[i]);
        }
    } evg{ev};
    if (g->timing) {
        HGX_HIP(hipEventCreate(&ev[0]));
        HGX_HIP(hipEventCreate(&ev[1]));
        HGX_HIP(hipEventRecord(ev[0], s));
    }
    HGX_HIP(hipMemsetAsync(ctr, 0, sizeof(u64) * cWords, s));

    SpArgs a{};
    a.A = A;
    a.mode = mode_of(o);
    a.want_type = o.link_type;
    a.inc_off = g->inc_off;
    a.inc_row = g->inc_row;
    a.inc_type = g->inc_type;
    a.tgt_off = g->tgt_off;
    a.tgt_idx = g->tgt_idx;
    a.link_atom = g->link_atom;
    a.keep = g->sib;
    a.w = lw ? lw->w : nullptr;
    a.dist = dist;
    a.stamp = stamp;
    a.pk = pk;
    a.ctr = ctr;
    a.cap = cap;

    auto read_words = [&]() {
        HGX_HIP(hipMemcpyAsync(host, ctr, sizeof(u64) * cWords, hipMemcpyDeviceToHost, s));
        HGX_HIP(hipStreamSynchronize(s));
        if (host[cOverflow]) fail(HGX_E_DEVICE, "hgx_shortest_paths: a work list overflowed (internal error)");
    };
    auto walk_grid = [](int64_t n_items) { return grid_for(n_items * 64, 256, 4096); };

    std::vector<int32_t> sg((size_t)(2 * K));
    std::vector<int64_t> lens((size_t)K), offs((size_t)K + 1);
    std::vector<u64> gd((size_t)K);
    r->path_off.assign(1, 0);
    for (int64_t c0 = 0; c0 < n_pairs; c0 += K) {
        const int64_t k = std::min<int64_t>(K, n_pairs - c0);
        a.K = k;
        std::memcpy(sg.data(), starts + c0, sizeof(int32_t) * (size_t)k);
        std::memcpy(sg.data() + k, goals + c0, sizeof(int32_t) * (size_t)k);
        HGX_HIP(hipMemcpyAsync(d_sg, sg.data(), sizeof(int32_t) * 2 * (size_t)k, hipMemcpyHostToDevice, s));
        a.starts = d_sg;
        a.goals = d_sg + k;
        HGX_HIP(hipMemsetAsync(ctr, 0, sizeof(u64) * 2, s));
        HGX_HIP(hipMemsetAsync(stamp, 0, sizeof(uint32_t) * (size_t)(k * A), s));
        hgx_sp_fill<<<grid_for(k * A, 256, 4096), 256, 0, s>>>(k * A, dist);
        HGX_CHECK_LAUNCH();
        int cur = 0;
        a.next = lists[cur];
        a.next_cnt = ctr + cCnt0 + cur;
        hgx_sp_seed<<<(unsigned)ceil_div(k, 64), 64, 0, s>>>(a);
        HGX_CHECK_LAUNCH();
        read_words();
        int64_t n = (int64_t)host[cCnt0 + cur];
        uint32_t round = 0;
        while (n > 0) {
            ++round;
            const int nxt = cur ^ 1;
            HGX_HIP(hipMemsetAsync(ctr + cCnt0 + nxt, 0, sizeof(u64), s));
            a.items = lists[cur];
            a.n_items = n;
            a.next = lists[nxt];
            a.next_cnt = ctr + cCnt0 + nxt;
            a.round = round;
            hgx_sp_walk<kRelax><<<walk_grid(n), 256, 0, s>>>(a);
            HGX_CHECK_LAUNCH();
            read_words();
            n = (int64_t)host[cCnt0 + nxt];
            cur = nxt;
            ++r->rounds;
        }

        // predecessors (rule R) inside every goal's radius, then the paths
        bool any = false;
        for (int64_t i = 0; i < k; ++i) any |= sg[i] != sg[k + i];
        if (any) {
            u64* pd = lists[1];   // the round lists are free now: [0] the sweep items, [1] pd (cap >= k * A)
            HGX_HIP(hipMemsetAsync(ctr + cCnt0, 0, sizeof(u64), s));
            HGX_HIP(hipMemsetAsync(ctr + cPlateau, 0, sizeof(u64), s));
            HGX_HIP(hipMemsetAsync(pd, 0xFF, sizeof(u64) * (size_t)(k * A), s));
            HGX_HIP(hipMemsetAsync(pk, 0xFF, sizeof(u64) * (size_t)(k * A), s));
            a.pd = pd;
            a.next = lists[0];
            a.next_cnt = ctr + cCnt0;
            hgx_sp_reached<<<grid_for(k * A, 256, 4096), 256, 0, s>>>(a);
            HGX_CHECK_LAUNCH();
            read_words();
            a.items = lists[0];
            a.n_items = (int64_t)host[cCnt0];
            a.next = nullptr;
            a.next_cnt = nullptr;
            a.use_lvl = 0;
            if (a.n_items > 0) {
                hgx_sp_walk<kPredDist><<<walk_grid(a.n_items), 256, 0, s>>>(a);
                HGX_CHECK_LAUNCH();
                hgx_sp_plateau<<<grid_for(k * A, 256, 4096), 256, 0, s>>>(a);
                HGX_CHECK_LAUNCH();
                read_words();
                if (host[cPlateau]) {   // zero / absorbed weights: order the equal-distance predecessors
                    a.use_lvl = 1;
                    for (;;) {
                        HGX_HIP(hipMemsetAsync(ctr + cChanged, 0, sizeof(u64), s));
                        hgx_sp_walk<kLevels><<<walk_grid(a.n_items), 256, 0, s>>>(a);
                        HGX_CHECK_LAUNCH();
                        read_words();
                        if (!host[cChanged]) break;
                    }
                }
                hgx_sp_walk<kPredKey><<<walk_grid(a.n_items), 256, 0, s>>>(a);
                HGX_CHECK_LAUNCH();
            }
        } else {
            HGX_HIP(hipMemsetAsync(pk, 0xFF, sizeof(u64) * (size_t)(k * A), s));
        }
        hgx_sp_path_len<<<(unsigned)ceil_div(k, 64), 64, 0, s>>>(a, d_gdist, d_len);
        HGX_CHECK_LAUNCH();
        HGX_HIP(hipMemcpyAsync(lens.data(), d_len, sizeof(int64_t) * (size_t)k, hipMemcpyDeviceToHost, s));
        HGX_HIP(hipMemcpyAsync(gd.data(), d_gdist, sizeof(u64) * (size_t)k, hipMemcpyDeviceToHost, s));
        HGX_HIP(hipStreamSynchronize(s));
        offs[0] = 0;
        for (int64_t i = 0; i < k; ++i) {
            if (lens[i] < 0) fail(HGX_E_DEVICE, "hgx_shortest_paths: broken predecessor chain (internal error)");
            offs[i + 1] = offs[i] + lens[i];
        }
        const int64_t total = offs[k];
        const size_t at = r->path_atoms.size();
        r->path_atoms.resize(at + (size_t)total);
        r->path_links.resize(at + (size_t)total);
        if (total > 0) {
            Scratch ps(g);
            int32_t* d_atoms = ps.get<int32_t>(total);
            int32_t* d_links = ps.get<int32_t>(total);
            HGX_HIP(hipMemcpyAsync(d_len, offs.data(), sizeof(int64_t) * (size_t)(k + 1), hipMemcpyHostToDevice, s));
            hgx_sp_path_write<<<(unsigned)ceil_div(k, 64), 64, 0, s>>>(a, d_len, d_atoms, d_links);
            HGX_CHECK_LAUNCH();
            HGX_HIP(hipMemcpyAsync(r->path_atoms.data() + at, d_atoms, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, s));
            HGX_HIP(hipMemcpyAsync(r->path_links.data() + at, d_links, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, s));
            HGX_HIP(hipStreamSynchronize(s));
        }
        for (int64_t i = 0; i < k; ++i) {
            const int64_t pi = c0 + i;
            r->path_off.push_back((int64_t)at + offs[i + 1]);
            double d;
            std::memcpy(&d, &gd[i], sizeof(d));
            r->dist[pi] = d;
            r->reached[pi] = gd[i] != kInfBits;
            if (goals[pi] < 0) {   // keep the rows on the device for the row readers
                hgx_sp_result::Row& row = r->rows[pi];
                row.dist = (u64*)g->alloc(sizeof(u64) * (size_t)A);
                row.pk = (u64*)g->alloc(sizeof(u64) * (size_t)A);
                HGX_HIP(hipMemcpyAsync(row.dist, dist + i * A, sizeof(u64) * (size_t)A, hipMemcpyDeviceToDevice, s));
                HGX_HIP(hipMemcpyAsync(row.pk, pk + i * A, sizeof(u64) * (size_t)A, hipMemcpyDeviceToDevice, s));
            }
        }
        HGX_HIP(hipStreamSynchronize(s));
    }
    read_words();
    r->expanded = (int64_t)host[cExpanded];
    r->entries = (int64_t)host[cEntries];
    r->relaxed = (int64_t)host[cRelaxed];
    r->improved = (int64_t)host[cImproved];
    // algorithmic bytes of the relaxation rounds: per item its word, d(a), d(goal) and the
    // incidence range; per entry its row, type, target offsets and weight; per edge its target and
    // distance; per improvement the atomic, the stamp, the incidence range and the queued item
    r->bytes = 40.0 * (double)r->expanded +
               (double)r->entries * (4.0 + (o.link_type >= 0 ? 4.0 : 0.0) + 16.0 + (lw ? 8.0 : 0.0)) +
               12.0 * (double)r->relaxed + 36.0 * (double)r->improved;
    if (g->timing) {
        HGX_HIP(hipEventRecord(ev[1], s));
        HGX_HIP(hipEventSynchronize(ev[1]));
        float ms = 0;
        HGX_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        r->ms_total = ms;
    }
}

}  // namespace

extern "C" {

int hgx_link_weights_create(hgx_graph* g, const double* w, hgx_link_weights** out) {
    HGX_API_BEGIN
    if (!g || !w || !out) fail(HGX_E_INVALID, "hgx_link_weights_create: null argument");
    *out = nullptr;
    if (g->shard) fail(HGX_E_UNSUPPORTED, "hgx_link_weights_create: not available on a partition shard");
    std::lock_guard<std::mutex> lk(g->mu);
    const int64_t M = g->M;
    std::vector<double> h((size_t)M);
    for (int64_t i = 0; i < M; ++i) {
        const double x = w[i];
        if (!(x >= 0.0) || std::isinf(x))   // NaN fails the comparison
            fail(HGX_E_INVALID, "hgx_link_weights_create: weight of link row " + std::to_string(i) +
                                    " is negative, NaN or infinite");
        h[(size_t)i] = x == 0.0 ? 0.0 : x;   // -0.0 is 0.0
    }
    HGX_HIP(hipSetDevice(g->device));
    std::unique_ptr<hgx_link_weights> lw(new hgx_link_weights());
    lw->device = g->device;
    lw->M = M;
    if (hipMalloc(&lw->w, sizeof(double) * (size_t)std::max<int64_t>(M, 1)) != hipSuccess) {
        (void)hipGetLastError();
        fail(HGX_E_NOMEM, "hgx_link_weights_create: device allocation failed");
    }
    hipError_t e = hipSuccess;
    if (M > 0) e = hipMemcpy(lw->w, h.data(), sizeof(double) * (size_t)M, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(lw->w);
        fail(HGX_E_DEVICE, std::string("hgx_link_weights_create: ") + hipGetErrorString(e));
    }
    *out = lw.release();
    HGX_API_END
}

void hgx_link_weights_free(hgx_link_weights* w) {
    if (!w) return;
    (void)hipSetDevice(w->device);
    if (w->w) (void)hipFree(w->w);
    delete w;
}

int hgx_shortest_paths(hgx_graph* g, const int32_t* starts, const int32_t* goals, int32_t n_pairs,
                       const hgx_algen_opts* opts, const hgx_link_weights* w, hgx_sp_result** out) {
    return hgx_shortest_paths_pred(g, starts, goals, n_pairs, opts, w, nullptr, out);
}

int hgx_shortest_paths_pred(hgx_graph* g, const int32_t* starts, const int32_t* goals, int32_t n_pairs,
                            const hgx_algen_opts* opts, const hgx_link_weights* w, hgx_link_predicate* p,
                            hgx_sp_result** out) {
    HGX_API_BEGIN
    shortest_paths_sib(g, starts, goals, n_pairs, opts, w, p, nullptr, out);
    HGX_API_END
}

}  // extern "C"

// hgx_shortest_paths, hgx_shortest_paths_pred (p null: the former) and hgx_shortest_paths_sib (ap null: the one before)
void hgx::shortest_paths_sib(hgx_graph* g, const int32_t* starts, const int32_t* goals, int32_t n_pairs,
                             const hgx_algen_opts* opts, const hgx_link_weights* w, hgx_link_predicate* p,
                             hgx_atom_predicate* ap, hgx_sp_result** out) {
    const std::string who = ap ? "hgx_shortest_paths_sib" : p ? "hgx_shortest_paths_pred" : "hgx_shortest_paths";
    if (!g || !out || n_pairs < 0 || (n_pairs > 0 && (!starts || !goals))) fail(HGX_E_INVALID, who + ": bad argument");
    *out = nullptr;
    if (g->shard) fail(HGX_E_UNSUPPORTED, who + ": not available on a partition shard");
    if (p) pred_check(g, p, opts, who.c_str());
    if (ap) apred_check(g, ap, who.c_str());
    hgx_algen_opts o = opts ? *opts : hgx_algen_opts{HGX_NO_TYPE, 1, 1, 0, 0};
    if (p) o.link_type = kLinkPredKey;   // the typed generator over the predicate's flags
    std::lock_guard<std::mutex> lk(g->mu);
    PredScope pred_scope(g, p);
    SibScope sib_scope(g, ap);
    for (int32_t i = 0; i < n_pairs; ++i) {
        if (starts[i] < 0 || starts[i] >= g->A) fail(HGX_E_INVALID, who + ": start out of range");
        if (goals[i] != HGX_NO_GOAL && (goals[i] < 0 || goals[i] >= g->A)) fail(HGX_E_INVALID, who + ": goal out of range");
    }
    if (w && (w->M != g->M || w->device != g->device))
        fail(HGX_E_INVALID, who + ": the weights were made for another link count or device");
    HGX_HIP(hipSetDevice(g->device));
    hgx_sp_result* r = new hgx_sp_result();
    struct Guard {   // error path: the graph mutex is held here, so release without re-locking
        hgx_sp_result* r;
        ~Guard() {
            if (!r) return;
            (void)hipStreamSynchronize(r->g->stream);
            release_rows(r);
            r->g->refs.fetch_sub(1);   // the caller still holds its own reference
            pred_release(r->pred);     // (likewise)
            apred_release(r->apred);
            delete r;
        }
    } guard{r};
    r->g = g;
    g->refs.fetch_add(1);
    r->pred = pred_ref(p);
    r->apred = apred_ref(ap);
    r->n_pairs = n_pairs;
    r->A = g->A;
    r->goals.assign(goals, goals + n_pairs);
    r->dist.assign((size_t)n_pairs, 0.0);
    r->reached.assign((size_t)n_pairs, 0);
    r->rows.resize((size_t)n_pairs);
    r->path_off.assign(1, 0);
    if (n_pairs > 0) sp_run(g, starts, goals, n_pairs, o, w, r);
    guard.r = nullptr;
    *out = r;
}

extern "C" {

int hgx_sp_result_info(const hgx_sp_result* r, int32_t* n_pairs) {
    HGX_API_BEGIN
    if (!r || !n_pairs) fail(HGX_E_INVALID, "hgx_sp_result_info: null argument");
    *n_pairs = r->n_pairs;
    HGX_API_END
}

int hgx_sp_result_distances(const hgx_sp_result* r, double* dist, uint8_t* reached) {
    HGX_API_BEGIN
    if (!r) fail(HGX_E_INVALID, "hgx_sp_result_distances: null result");
    if (dist && r->n_pairs) std::memcpy(dist, r->dist.data(), sizeof(double) * (size_t)r->n_pairs);
    if (reached && r->n_pairs) std::memcpy(reached, r->reached.data(), (size_t)r->n_pairs);
    HGX_API_END
}

int hgx_sp_result_path(hgx_sp_result* r, int32_t pair, int32_t* atoms, int32_t* links, int64_t cap, int64_t* n_out) {
    HGX_API_BEGIN
    if (!r || !n_out || cap < 0 || (cap > 0 && !atoms)) fail(HGX_E_INVALID, "hgx_sp_result_path: bad argument");
    if (pair < 0 || pair >= r->n_pairs) fail(HGX_E_INVALID, "hgx_sp_result_path: pair out of range");
    const int64_t o = r->path_off[(size_t)pair], n = r->path_off[(size_t)pair + 1] - o;
    *n_out = n;
    const int64_t k = std::min(n, cap);
    if (k > 0) std::memcpy(atoms, r->path_atoms.data() + o, sizeof(int32_t) * (size_t)k);
    if (k > 1 && links) std::memcpy(links, r->path_links.data() + o + 1, sizeof(int32_t) * (size_t)(k - 1));
    HGX_API_END
}

}  // extern "C"

namespace {
// D2H copy of a row range of an HGX_NO_GOAL pair (graph mutex taken here).
void read_row(hgx_sp_result* r, int32_t pair, int64_t first, int64_t n, bool keys, u64* out, const char* who) {
    if (!r || n < 0 || (n > 0 && !out)) fail(HGX_E_INVALID, std::string(who) + ": bad argument");
    if (pair < 0 || pair >= r->n_pairs) fail(HGX_E_INVALID, std::string(who) + ": pair out of range");
    if (r->goals[(size_t)pair] != HGX_NO_GOAL) fail(HGX_E_NOTFOUND, std::string(who) + ": not an HGX_NO_GOAL pair");
    if (first < 0 || first > r->A || n > r->A - first) fail(HGX_E_INVALID, std::string(who) + ": atom range out of bounds");
    if (n == 0) return;
    hgx_graph* g = r->g;
    std::lock_guard<std::mutex> lk(g->mu);
    HGX_HIP(hipSetDevice(g->device));
    const u64* src = keys ? r->rows[(size_t)pair].pk : r->rows[(size_t)pair].dist;
    HGX_HIP(hipMemcpyAsync(out, src + first, sizeof(u64) * (size_t)n, hipMemcpyDeviceToHost, g->stream));
    HGX_HIP(hipStreamSynchronize(g->stream));
}
}  // namespace

extern "C" {

int hgx_sp_result_distance_row(hgx_sp_result* r, int32_t pair, int64_t first, int64_t n, double* out) {
    HGX_API_BEGIN
    read_row(r, pair, first, n, false, (u64*)out, "hgx_sp_result_distance_row");   // the words are the doubles' bits
    HGX_API_END
}

int hgx_sp_result_predecessor_row(hgx_sp_result* r, int32_t pair, int64_t first, int64_t n, int32_t* pred_atom,
                                  int32_t* pred_link) {
    HGX_API_BEGIN
    std::vector<u64> keys((size_t)std::max<int64_t>(n, 0));
    read_row(r, pair, first, n, true, keys.data(), "hgx_sp_result_predecessor_row");
    for (int64_t i = 0; i < n; ++i) {   // no predecessor: all ones = (-1, -1)
        if (pred_atom) pred_atom[i] = (int32_t)(uint32_t)(keys[(size_t)i] >> 32);
        if (pred_link) pred_link[i] = (int32_t)(uint32_t)keys[(size_t)i];
    }
    HGX_API_END
}

int hgx_sp_result_stats(const hgx_sp_result* r, int64_t* rounds, int64_t* expanded, int64_t* relaxed, int64_t* improved,
                        double* ms_total, double* bytes) {
    HGX_API_BEGIN
    if (!r) fail(HGX_E_INVALID, "hgx_sp_result_stats: null result");
    if (rounds) *rounds = r->rounds;
    if (expanded) *expanded = r->expanded;
    if (relaxed) *relaxed = r->relaxed;
    if (improved) *improved = r->improved;
    if (ms_total) *ms_total = r->ms_total;
    if (bytes) *bytes = r->bytes;
    HGX_API_END
}

void hgx_sp_result_free(hgx_sp_result* r) {
    if (!r) return;
    hgx_graph* g = r->g;
    if (g) {
        std::lock_guard<std::mutex> lk(g->mu);
        (void)hipSetDevice(g->device);
        release_rows(r);
    }
    hgx_link_predicate* const pred = r->pred;
    hgx_atom_predicate* const apred = r->apred;
    delete r;
    pred_release(pred);
    apred_release(apred);
    if (g) graph_release(g);
}

}  // extern "C"
