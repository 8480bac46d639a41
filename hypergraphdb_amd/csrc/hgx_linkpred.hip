// hgx_linkpred.hip -- link predicates of the traversals (include/hgx_linkpred.h).
//
// Replaces the linkPredicate of a DefaultALGenerator: generate() calls linkPredicate.satisfies(graph, link) once
// per incident link and nothing else (C/algorithms/DefaultALGenerator.java:300-308), so the predicate is a
// property of the link row alone.  It is evaluated once per link row when the object is made, not once per
// incidence entry per level inside the traversal kernels:
//   hgx_linkpred_eval    -- one lane per link row: the row's offset pair, its first 8 targets into registers
//        (longer rows loop over the rest in memory) unless the program has only type / arity literals, its type
//        when a type literal is met; then the program, the walk over terms and literals of the negation
//        filter (hgx_not_dev.h: the tree is the inside of one negation, so P = !negations_keep); flag[row] = P;
//   hgx_linkpred_project -- inc_flag[i] = flag[inc_row[i]]: the flags in incidence order.
// flag / inc_flag are int32 so that every traversal kernel reads them in place of link_type / inc_type with the
// type key 1 (PredScope, hgx_internal.h), byte for byte the kernels of a typed traversal.
#include "hgx_not_dev.h"

namespace hgx {

namespace {

struct PredArgs {
    NotDev prog;                 // term_off = {0, n_terms}: one "negation"
    int64_t M;
    const int64_t* tgt_off;
    const int32_t* tgt_idx;
    const int32_t* link_type;
    int32_t needs_targets;       // a literal reads targets (else only tgt_off and link_type are read)
    int32_t* flag;               // [M]
    unsigned long long* ctr;     // [4] rows satisfied, targets read, types read
};

__global__ void __launch_bounds__(256) hgx_linkpred_eval(PredArgs a) {
    u64 sat = 0, targets_read = 0, types_read = 0;
    for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < a.M; row += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = a.tgt_off[row];
        Link L;
        L.tg = a.tgt_idx + b;
        L.n = (int32_t)(a.tgt_off[row + 1] - b);
        if (a.needs_targets) {
#pragma unroll
            for (int k = 0; k < 8; ++k) L.r[k] = k < L.n ? L.tg[k] : -1;
            targets_read += (u64)L.n;
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) L.r[k] = -1;
        }
        int32_t type = INT32_MIN;
        const bool p = !negations_keep(a.prog, 0, 1, L, a.link_type, row, type, types_read);
        a.flag[row] = p ? 1 : 0;
        sat += p ? 1 : 0;
    }
    wave_add(a.ctr + 0, sat);
    wave_add(a.ctr + 1, targets_read);
    wave_add(a.ctr + 2, types_read);
}

__global__ void __launch_bounds__(256) hgx_linkpred_project(int64_t I, const int32_t* __restrict__ inc_row,
                                                            const int32_t* __restrict__ flag,
                                                            int32_t* __restrict__ inc_flag) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < I; i += (int64_t)gridDim.x * blockDim.x)
        inc_flag[i] = flag[inc_row[i]];
}

}  // namespace

void linkpred_validate(int64_t A, int64_t n_terms, NotProgram& p, bool* needs_targets) {
    const char* who = "hgx_link_predicate_create: ";
    *needs_targets = false;
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
            std::string why;
            if (const int rc = not_check_literal(A, p, l, why))
                fail(rc, std::string(who) + "term " + std::to_string(t) + " literal " + std::to_string(l - p.lit_off[t]) + why);
            const int32_t kind = p.lit[4 * l];
            if (kind != HGX_NOT_TYPE && kind != HGX_NOT_ARITY) *needs_targets = true;
        }
}

void pred_release(hgx_link_predicate* p) {
    if (!p || p->refs.fetch_sub(1) != 1) return;
    hgx_graph* root = p->root;
    (void)hipSetDevice(root->device);
    if (p->flag) (void)hipFree(p->flag);
    if (p->inc_flag) (void)hipFree(p->inc_flag);
    for (YieldList& y : p->ylists) {
        (void)hipFree(y.off);
        (void)hipFree(y.row);
    }
    for (YieldAdj& y : p->yadjs) {
        if (y.off) (void)hipFree(y.off);
        if (y.tgt) (void)hipFree(y.tgt);
        if (y.lnk) (void)hipFree(y.lnk);
    }
    delete p;
    graph_release(root);
}

void pred_check(const hgx_graph* g, const hgx_link_predicate* p, const hgx_algen_opts* opts, const char* who) {
    if (p->root != (g->base ? g->base : g))
        fail(HGX_E_INVALID, std::string(who) + ": the link predicate was made on another graph");
    if (opts && opts->link_type != HGX_NO_TYPE)
        fail(HGX_E_INVALID, std::string(who) + ": opts->link_type must be HGX_NO_TYPE with a link predicate "
                                               "(a type belongs inside the predicate)");
}

}  // namespace hgx

using namespace hgx;

extern "C" {

int hgx_link_predicate_create(hgx_graph* g, int64_t n_terms, const int64_t* lit_off, const int32_t* lit,
                              const int32_t* ops, int64_t n_ops, hgx_link_predicate** out) {
    HGX_API_BEGIN
    if (!g || !out) fail(HGX_E_INVALID, "hgx_link_predicate_create: null argument");
    *out = nullptr;
    if (g->shard) fail(HGX_E_UNSUPPORTED, "hgx_link_predicate_create: not available on a partition shard");
    NotProgram np;
    np.lit_off = lit_off;
    np.lit = lit;
    np.ops = ops;
    np.n_ops = n_ops;
    bool needs_targets = false;
    linkpred_validate(g->A, n_terms, np, &needs_targets);

    std::lock_guard<std::mutex> lk(g->mu);
    HGX_HIP(hipSetDevice(g->device));
    hipStream_t s = g->stream;
    hgx_graph* root = g->base ? g->base : g;
    const int64_t M = g->M, I = g->I;
    hgx_link_predicate* p = new hgx_link_predicate();
    p->root = root;
    root->refs.fetch_add(1);
    struct Guard {
        hgx_link_predicate* p;
        ~Guard() { pred_release(p); }
    } guard{p};
    p->M = M;
    p->I = I;
    HGX_HIP(hipMalloc(&p->flag, sizeof(int32_t) * (size_t)std::max<int64_t>(M, 1)));
    HGX_HIP(hipMalloc(&p->inc_flag, sizeof(int32_t) * (size_t)std::max<int64_t>(I, 1)));

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
    u64* d_ctr = (u64*)w.take(sizeof(u64) * 4);
    HGX_HIP(hipMemcpyAsync(d_toff, toff, sizeof(toff), hipMemcpyHostToDevice, s));
    HGX_HIP(hipMemcpyAsync(d_lo, n_terms > 0 ? lit_off : &zero, b_lo, hipMemcpyHostToDevice, s));
    if (b_lit) HGX_HIP(hipMemcpyAsync(d_lit, lit, b_lit, hipMemcpyHostToDevice, s));
    if (b_ops) HGX_HIP(hipMemcpyAsync(d_ops, ops, b_ops, hipMemcpyHostToDevice, s));
    HGX_HIP(hipMemsetAsync(d_ctr, 0, sizeof(u64) * 4, s));

    PredArgs a{};
    a.prog.term_off = d_toff;
    a.prog.lit_off = d_lo;
    a.prog.lit = d_lit;
    a.prog.ops = d_ops;
    a.M = M;
    a.tgt_off = g->tgt_off;
    a.tgt_idx = g->tgt_idx;
    a.link_type = g->link_type;
    a.needs_targets = needs_targets ? 1 : 0;
    a.flag = p->flag;
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
    if (M > 0) {
        hgx_linkpred_eval<<<grid_for(M, 256), 256, 0, s>>>(a);
        HGX_CHECK_LAUNCH();
    }
    if (I > 0) {
        hgx_linkpred_project<<<grid_for(I, 256), 256, 0, s>>>(I, g->inc_row, p->flag, p->inc_flag);
        HGX_CHECK_LAUNCH();
    }
    if (g->timing) HGX_HIP(hipEventRecord(ev[1], s));
    u64 ctr[4] = {0, 0, 0, 0};
    HGX_HIP(hipMemcpyAsync(ctr, d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, s));
    HGX_HIP(hipStreamSynchronize(s));   // (the host arrays of the program are the caller's: done with them here)
    p->n_sat = (int64_t)ctr[0];
    if (g->timing) {
        float ms = 0;
        HGX_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        p->ms_eval = ms;
    }
    // eval: the offset pairs (streamed: 8 bytes a row), the targets and types it read, the flags; project: inc_row,
    // one flag read and one flag write per entry
    p->bytes_eval = 8.0 * (double)(M + 1) + 4.0 * (double)ctr[1] + 4.0 * (double)ctr[2] + 4.0 * (double)M + 12.0 * (double)I;
    guard.p = nullptr;
    *out = p;
    HGX_API_END
}

void hgx_link_predicate_free(hgx_link_predicate* p) { pred_release(p); }

int hgx_link_predicate_info(const hgx_link_predicate* p, int64_t* num_links, int64_t* num_satisfied, double* ms_eval,
                            double* bytes_eval) {
    HGX_API_BEGIN
    if (!p) fail(HGX_E_INVALID, "hgx_link_predicate_info: null predicate");
    if (num_links) *num_links = p->M;
    if (num_satisfied) *num_satisfied = p->n_sat;
    if (ms_eval) *ms_eval = p->ms_eval;
    if (bytes_eval) *bytes_eval = p->bytes_eval;
    HGX_API_END
}

int hgx_link_predicate_flags(hgx_link_predicate* p, int64_t first, int64_t n, uint8_t* out) {
    HGX_API_BEGIN
    if (!p || n < 0 || (n > 0 && !out)) fail(HGX_E_INVALID, "hgx_link_predicate_flags: bad argument");
    if (first < 0 || first > p->M || n > p->M - first)
        fail(HGX_E_INVALID, "hgx_link_predicate_flags: link row range out of bounds");
    if (n == 0) return HGX_OK;
    hgx_graph* g = p->root;
    std::vector<int32_t> h((size_t)n);
    {
        std::lock_guard<std::mutex> lk(g->mu);
        HGX_HIP(hipSetDevice(g->device));
        HGX_HIP(hipMemcpyAsync(h.data(), p->flag + first, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, g->stream));
        HGX_HIP(hipStreamSynchronize(g->stream));
    }
    for (int64_t i = 0; i < n; ++i) out[i] = h[(size_t)i] ? 1 : 0;
    HGX_API_END
}

}  // extern "C"
