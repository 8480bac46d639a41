// hgx_sibling.hip -- sibling predicates of the batched traversals (include/hgx_sibling.h).
//
// Replaces the siblingPredicate of a DefaultALGenerator: the iterator drops every target h of generate(src) for
// which siblingPredicate.satisfies(graph, h) is false (C/algorithms/DefaultALGenerator.java:120-150, 207-237), so
// the predicate is a property of the atom alone.  It is evaluated once per atom when the object is made, one bit
// an atom, not once per yielded target inside the traversal kernels:
//   hgx_sibling_eval     -- one lane per atom: the atom's type, then the program, the walk over terms and type
//        literals of the negation filter (hgx_not_dev.h: the tree is the inside of one negation, so
//        P = !negations_keep); the wave's 64 verdicts are one ballot word, stored by lane 0;
//        its MASK instantiation makes the same words from one byte an atom (hgx_atom_predicate_create_mask);
//   hgx_sibling_saturate -- the batched BFS's prologue, a wave per 64 atoms: every atom whose bit is 0 becomes
//        visited by every traversal of the batch (vis row = the full mask, ever and full bits) before level 1, so
//        no level kind produces it as new and none of the level kernels reads the bits.
// The weighted shortest paths test the target's bit in hgx_sp_walk (hgx_paths.hip).
#include "hgx_not_dev.h"

namespace hgx {

namespace {

struct SibArgs {
    NotDev prog;                 // term_off = {0, n_terms}: one "negation"
    int64_t A;
    const int32_t* atom_type;    // [A]  (eval)
    const uint8_t* keep;         // [A]  (pack)
    u64* bits;                   // [ceil(A / 64)] written; the words behind them are zero
    u64* ctr;                    // [1] atoms kept
};

// A wave owns the 64 atoms of one word at a time; the lanes past A vote 0 (the tail word's high bits stay 0).
template <bool MASK>
__global__ void __launch_bounds__(256) hgx_sibling_eval(SibArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t nw = (a.A + 63) >> 6;
    u64 kept = 0;
    for (int64_t w = wave; w < nw; w += nwave) {   // wave-uniform
        const int64_t atom = w * 64 + lane;
        bool p = false;
        if (atom < a.A) {
            if (MASK) {
                p = a.keep[atom] != 0;
            } else {
                Link L;
                L.tg = nullptr;
                L.n = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) L.r[k] = -1;
                int32_t type = a.atom_type[atom];   // handed over: a type literal reads nothing more
                u64 types_read = 0;
                p = !negations_keep(a.prog, 0, 1, L, a.atom_type, atom, type, types_read);
            }
        }
        const u64 word = __ballot(p);
        if (lane == 0) {
            a.bits[w] = word;
            kept += (u64)__popcll(word);
        }
    }
    wave_add(a.ctr, kept);
}

struct FullWords {
    u64 w[16];
};

// A wave per word of the bitmap, i.e. per 64 atoms: a word without a failing atom costs its one load; otherwise lane 0
// ORs the failing atoms into the ever / full words and the lanes store the full mask over the failing atoms' rows,
// which lie in one block of 64 W words (consecutive lanes, consecutive words).  Runs after hgx_seed on the same
// stream and before any level, so nothing else writes these; the tail word's bits past A are masked off, so no row
// past A is written.
__global__ void __launch_bounds__(256) hgx_sibling_saturate(const u64* __restrict__ keep, int64_t A, int lgW, FullWords fm,
                                                            u64* __restrict__ vis, u64* __restrict__ ever,
                                                            u64* __restrict__ full) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t nw = (A + 63) >> 6;
    const int wmask = (1 << lgW) - 1, row_words = 64 << lgW;
    for (int64_t j = wave; j < nw; j += nwave) {   // wave-uniform
        u64 m = ~keep[j];
        if (j == nw - 1 && (A & 63)) m &= (1ull << (A & 63)) - 1ull;
        if (m == 0) continue;
        if (lane == 0) {
            ever[j] |= m;
            full[j] |= m;
        }
        u64* rows = vis + ((j * 64) << lgW);
        for (int k = lane; k < row_words; k += 64)
            if ((m >> (k >> lgW)) & 1ull) rows[k] = fm.w[k & wmask];
    }
}

size_t bits_bytes(int64_t A) { return sizeof(u64) * (size_t)(A / 64 + 2); }

// The object of both constructors: a reference on the snapshot, the zeroed words.  The caller holds g->mu.
hgx_atom_predicate* apred_new(hgx_graph* g) {
    hgx_graph* root = g->base ? g->base : g;
    hgx_atom_predicate* p = new hgx_atom_predicate();
    p->root = root;
    root->refs.fetch_add(1);
    p->A = g->A;
    return p;
}

struct ApredGuard {
    hgx_atom_predicate* p;
    ~ApredGuard() { apred_release(p); }
};

// Evaluates a (typed program or byte mask) into p->bits on g's stream and waits; fills the statistics.
template <bool MASK>
void apred_eval(hgx_graph* g, hgx_atom_predicate* p, SibArgs& a, u64* d_ctr) {
    hipStream_t s = g->stream;
    const int64_t A = g->A;
    HGX_HIP(hipMalloc(&p->bits, bits_bytes(A)));
    HGX_HIP(hipMemsetAsync(p->bits, 0, bits_bytes(A), s));
    HGX_HIP(hipMemsetAsync(d_ctr, 0, sizeof(u64), s));
    a.A = A;
    a.bits = p->bits;
    a.ctr = d_ctr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EvGuard {
        hipEvent_t* ev;
        ~EvGuard() {
            for (int k = 0; k < 2; ++k)
                if (ev[k]) (void)hipEventDestroy(ev[k]);
        }
    } ev_guard{ev};
    if (g->timing) {
        HGX_HIP(hipEventCreate(&ev[0]));
        HGX_HIP(hipEventCreate(&ev[1]));
        HGX_HIP(hipEventRecord(ev[0], s));
    }
    if (A > 0) {
        hgx_sibling_eval<MASK><<<grid_for(ceil_div(A, 64) * 64, 256), 256, 0, s>>>(a);
        HGX_CHECK_LAUNCH();
    }
    if (g->timing) HGX_HIP(hipEventRecord(ev[1], s));
    u64 kept = 0;
    HGX_HIP(hipMemcpyAsync(&kept, d_ctr, sizeof(u64), hipMemcpyDeviceToHost, s));
    HGX_HIP(hipStreamSynchronize(s));   // (the host arrays are the caller's: done with them here)
    p->n_kept = (int64_t)kept;
    if (g->timing) {
        float ms = 0;
        HGX_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        p->ms_eval = ms;
    }
    // one type (4 bytes) or one byte an atom read, one word per 64 atoms written
    p->bytes_eval = (MASK ? 1.0 : 4.0) * (double)A + 8.0 * (double)ceil_div(A, 64);
}

}  // namespace

void atompred_validate(int64_t A, int64_t n_terms, NotProgram& p) {
    const char* who = "hgx_atom_predicate_create: ";
    p.n_negs = 1;
    p.n_terms = n_terms;
    p.n_lits = 0;
    if (n_terms < 0) fail(HGX_E_INVALID, std::string(who) + "negative n_terms");
    if (n_terms > 0) {
        if (!p.lit_off) fail(HGX_E_INVALID, std::string(who) + "null lit_off");
        if (p.lit_off[0] != 0) fail(HGX_E_INVALID, std::string(who) + "lit_off[0] is not 0");
        for (int64_t t = 0; t < n_terms; ++t)
            if (p.lit_off[t + 1] < p.lit_off[t])
                fail(HGX_E_INVALID, std::string(who) + "term " + std::to_string(t) + ": lit_off decreases");
        p.n_lits = p.lit_off[n_terms];
    }
    if (n_terms > INT32_MAX || p.n_lits > INT32_MAX) fail(HGX_E_UNSUPPORTED, std::string(who) + "predicate too large");
    if (p.n_lits > 0 && !p.lit) fail(HGX_E_INVALID, std::string(who) + "null lit");
    if (p.n_ops < 0 || p.n_ops > INT32_MAX || (p.n_ops > 0 && !p.ops)) fail(HGX_E_INVALID, std::string(who) + "bad ops");
    for (int64_t t = 0; t < n_terms; ++t)
        for (int64_t l = p.lit_off[t]; l < p.lit_off[t + 1]; ++l) {
            const std::string where = "term " + std::to_string(t) + " literal " + std::to_string(l - p.lit_off[t]);
            std::string why;
            if (const int rc = not_check_literal(A, p, l, why)) fail(rc, std::string(who) + where + why);
            if (p.lit[4 * l] != HGX_NOT_TYPE)
                fail(HGX_E_UNSUPPORTED, std::string(who) + where + ": only type literals are evaluated on atoms "
                                                                   "(use hgx_atom_predicate_create_mask)");
        }
}

void atom_types_validate(int64_t A, int64_t M, const int32_t* atom_type, const int32_t* link_atom,
                         const int32_t* link_type) {
    const char* who = "hgx_graph_set_atom_types: ";
    for (int64_t a = 0; a < A; ++a)
        if (atom_type[a] < 0) fail(HGX_E_INVALID, std::string(who) + "atom " + std::to_string(a) + " has a negative type");
    for (int64_t r = 0; r < M; ++r) {
        const int32_t la = link_atom[r];
        if (la < 0 || la >= A || link_type[r] < 0) continue;   // (a row without a type pins nothing)
        if (atom_type[la] != link_type[r])
            fail(HGX_E_INVALID, std::string(who) + "link row " + std::to_string(r) + " (atom " + std::to_string(la) +
                                    ") has the type " + std::to_string(link_type[r]) + " on the snapshot, not " +
                                    std::to_string(atom_type[la]));
    }
}

void apred_release(hgx_atom_predicate* p) {
    if (!p || p->refs.fetch_sub(1) != 1) return;
    hgx_graph* root = p->root;
    (void)hipSetDevice(root->device);
    if (p->bits) (void)hipFree(p->bits);
    if (p->typed) root->type_preds.fetch_sub(1);
    delete p;
    graph_release(root);
}

void apred_check(const hgx_graph* g, const hgx_atom_predicate* ap, const char* who) {
    if (ap->root != (g->base ? g->base : g))
        fail(HGX_E_INVALID, std::string(who) + ": the atom predicate was made on another graph");
}

void sib_saturate(const u64* keep, int64_t A, int W, const u64* fm, u64* vis, u64* ever, u64* full, hipStream_t s) {
    if (A <= 0) return;
    FullWords f{};
    for (int w = 0; w < W && w < 16; ++w) f.w[w] = fm[w];
    int lgW = 0;
    while ((1 << lgW) < W) ++lgW;
    hgx_sibling_saturate<<<grid_for(ceil_div(A, 64) * 64, 256), 256, 0, s>>>(keep, A, lgW, f, vis, ever, full);
    HGX_CHECK_LAUNCH();
}

}  // namespace hgx

using namespace hgx;

extern "C" {

int hgx_graph_set_atom_types(hgx_graph* g, const int32_t* atom_type) {
    HGX_API_BEGIN
    if (!g) fail(HGX_E_INVALID, "hgx_graph_set_atom_types: null graph");
    if (g->shard) fail(HGX_E_UNSUPPORTED, "hgx_graph_set_atom_types: not available on a partition shard");
    if (g->base) fail(HGX_E_INVALID, "hgx_graph_set_atom_types: set the types on the snapshot, not on one of its contexts");
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->type_preds.load() > 0)
        fail(HGX_E_INVALID, "hgx_graph_set_atom_types: an atom predicate made from the atom types is still alive");
    HGX_HIP(hipSetDevice(g->device));
    hipStream_t s = g->stream;
    int32_t* fresh = nullptr;
    if (atom_type) {
        const int64_t A = g->A, M = g->M;
        std::vector<int32_t> la((size_t)M), ty((size_t)M);
        if (M > 0) {
            HGX_HIP(hipMemcpyAsync(la.data(), g->link_atom, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, s));
            HGX_HIP(hipMemcpyAsync(ty.data(), g->link_type, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, s));
            HGX_HIP(hipStreamSynchronize(s));
        }
        atom_types_validate(A, M, atom_type, la.data(), ty.data());
        HGX_HIP(hipMalloc(&fresh, sizeof(int32_t) * (size_t)std::max<int64_t>(A, 1)));
        hipError_t e = hipSuccess;
        if (A > 0) e = hipMemcpyAsync(fresh, atom_type, sizeof(int32_t) * (size_t)A, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hipFree(fresh);
            HGX_HIP(e);
        }
    }
    if (g->atom_type) (void)hipFree(g->atom_type);   // (every evaluation that read it has been waited for)
    g->atom_type = fresh;
    g->atom_index.reset();   // (include/hgx_atoms.h: the next scan over the atoms builds it from the new column)
    HGX_API_END
}

int hgx_atom_predicate_create(hgx_graph* g, int64_t n_terms, const int64_t* lit_off, const int32_t* lit,
                              const int32_t* ops, int64_t n_ops, hgx_atom_predicate** out) {
    HGX_API_BEGIN
    if (!g || !out) fail(HGX_E_INVALID, "hgx_atom_predicate_create: null argument");
    *out = nullptr;
    if (g->shard) fail(HGX_E_UNSUPPORTED, "hgx_atom_predicate_create: not available on a partition shard");
    NotProgram np;
    np.lit_off = lit_off;
    np.lit = lit;
    np.ops = ops;
    np.n_ops = n_ops;
    atompred_validate(g->A, n_terms, np);

    hgx_graph* root = g->base ? g->base : g;
    std::lock_guard<std::mutex> lk(g->mu);
    // the column is the snapshot's: a context holds the snapshot's mutex too while it reads it (contexts first,
    // then the snapshot; nothing takes them the other way round)
    std::unique_lock<std::mutex> rlk;
    if (root != g) rlk = std::unique_lock<std::mutex>(root->mu);
    if (!root->atom_type)
        fail(HGX_E_UNSUPPORTED, "hgx_atom_predicate_create: the snapshot has no atom types (hgx_graph_set_atom_types)");
    HGX_HIP(hipSetDevice(g->device));
    hipStream_t s = g->stream;
    hgx_atom_predicate* p = apred_new(g);
    ApredGuard guard{p};
    p->typed = true;
    root->type_preds.fetch_add(1);

    // the program in pool memory: {0, n_terms}, lit_off (a lone 0 for a predicate without terms), lit, ops
    PoolScratch w{g, {}};
    const int64_t toff[2] = {0, n_terms};
    const int64_t zero = 0;
    const size_t b_lo = sizeof(int64_t) * (size_t)(n_terms + 1), b_lit = sizeof(int32_t) * 4 * (size_t)np.n_lits,
                 b_ops = sizeof(int32_t) * (size_t)n_ops;
    int64_t* d_toff = (int64_t*)w.take(sizeof(toff));
    int64_t* d_lo = (int64_t*)w.take(b_lo);
    int4* d_lit = (int4*)w.take(std::max<size_t>(b_lit, 16));
    int32_t* d_ops = (int32_t*)w.take(std::max<size_t>(b_ops, 4));
    u64* d_ctr = (u64*)w.take(sizeof(u64));
    HGX_HIP(hipMemcpyAsync(d_toff, toff, sizeof(toff), hipMemcpyHostToDevice, s));
    HGX_HIP(hipMemcpyAsync(d_lo, n_terms > 0 ? lit_off : &zero, b_lo, hipMemcpyHostToDevice, s));
    if (b_lit) HGX_HIP(hipMemcpyAsync(d_lit, lit, b_lit, hipMemcpyHostToDevice, s));
    if (b_ops) HGX_HIP(hipMemcpyAsync(d_ops, ops, b_ops, hipMemcpyHostToDevice, s));
    SibArgs a{};
    a.prog.term_off = d_toff;
    a.prog.lit_off = d_lo;
    a.prog.lit = d_lit;
    a.prog.ops = d_ops;
    a.atom_type = root->atom_type;
    apred_eval<false>(g, p, a, d_ctr);
    guard.p = nullptr;
    *out = p;
    HGX_API_END
}

int hgx_atom_predicate_create_mask(hgx_graph* g, const uint8_t* keep, hgx_atom_predicate** out) {
    HGX_API_BEGIN
    if (!g || !out || (g->A > 0 && !keep)) fail(HGX_E_INVALID, "hgx_atom_predicate_create_mask: null argument");
    *out = nullptr;
    if (g->shard) fail(HGX_E_UNSUPPORTED, "hgx_atom_predicate_create_mask: not available on a partition shard");
    std::lock_guard<std::mutex> lk(g->mu);
    HGX_HIP(hipSetDevice(g->device));
    hgx_atom_predicate* p = apred_new(g);
    ApredGuard guard{p};
    PoolScratch w{g, {}};
    const size_t nb = (size_t)std::max<int64_t>(g->A, 1);
    uint8_t* d_keep = (uint8_t*)w.take(nb);
    u64* d_ctr = (u64*)w.take(sizeof(u64));
    if (g->A > 0) HGX_HIP(hipMemcpyAsync(d_keep, keep, (size_t)g->A, hipMemcpyHostToDevice, g->stream));
    SibArgs a{};
    a.keep = d_keep;
    apred_eval<true>(g, p, a, d_ctr);
    guard.p = nullptr;
    *out = p;
    HGX_API_END
}

void hgx_atom_predicate_free(hgx_atom_predicate* p) { apred_release(p); }

int hgx_atom_predicate_info(const hgx_atom_predicate* p, int64_t* num_atoms, int64_t* num_kept, double* ms_eval,
                            double* bytes_eval) {
    HGX_API_BEGIN
    if (!p) fail(HGX_E_INVALID, "hgx_atom_predicate_info: null predicate");
    if (num_atoms) *num_atoms = p->A;
    if (num_kept) *num_kept = p->n_kept;
    if (ms_eval) *ms_eval = p->ms_eval;
    if (bytes_eval) *bytes_eval = p->bytes_eval;
    HGX_API_END
}

int hgx_atom_predicate_flags(hgx_atom_predicate* p, int64_t first, int64_t n, uint8_t* out) {
    HGX_API_BEGIN
    if (!p || n < 0 || (n > 0 && !out)) fail(HGX_E_INVALID, "hgx_atom_predicate_flags: bad argument");
    if (first < 0 || first > p->A || n > p->A - first)
        fail(HGX_E_INVALID, "hgx_atom_predicate_flags: atom range out of bounds");
    if (n == 0) return HGX_OK;
    hgx_graph* g = p->root;
    const int64_t w0 = first >> 6, w1 = (first + n - 1) >> 6;   // w1 < ceil(A / 64)
    std::vector<u64> h((size_t)(w1 - w0 + 1));
    {
        std::lock_guard<std::mutex> lk(g->mu);
        HGX_HIP(hipSetDevice(g->device));
        HGX_HIP(hipMemcpyAsync(h.data(), p->bits + w0, sizeof(u64) * h.size(), hipMemcpyDeviceToHost, g->stream));
        HGX_HIP(hipStreamSynchronize(g->stream));
    }
    for (int64_t i = 0; i < n; ++i) {
        const int64_t a = first + i;
        out[i] = (uint8_t)((h[(size_t)((a >> 6) - w0)] >> (a & 63)) & 1ull);
    }
    HGX_API_END
}

int hgx_bfs_batch_sib(hgx_graph* g, const int32_t* seeds, int32_t n_seeds, int32_t max_depth,
                      const hgx_algen_opts* opts, hgx_link_predicate* link_pred, hgx_atom_predicate* ap,
                      hgx_bfs_result** out) {
    HGX_API_BEGIN
    bfs_batch_sib(g, seeds, n_seeds, max_depth, opts, link_pred, ap, out);
    HGX_API_END
}

int hgx_shortest_paths_sib(hgx_graph* g, const int32_t* starts, const int32_t* goals, int32_t n_pairs,
                           const hgx_algen_opts* opts, const hgx_link_weights* w, hgx_link_predicate* link_pred,
                           hgx_atom_predicate* ap, hgx_sp_result** out) {
    HGX_API_BEGIN
    shortest_paths_sib(g, starts, goals, n_pairs, opts, w, link_pred, ap, out);
    HGX_API_END
}

}  // extern "C"
