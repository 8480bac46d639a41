// hgx_not.hip -- negated predicates on the clause hits of a DNF batch (hgx_pattern_batch_dnf_not).
//
// Replaces the PredicateBasedFilter that AndToQuery.getQuery (C/query/cond2qry/AndToQuery.java:126-135,
// :279-294) puts over the intersection of an And for every sub-condition without a query translation -- a
// Not is one: toDNF (C/query/cond2qry/ExpressionBasedQuery.java:94-167) keeps it as an opaque leaf -- and
// Not.satisfies = !negated.satisfies(graph, candidate) (C/query/Not.java:33-36).  The negated tree is
// evaluated on the candidate link with the leaves' raw satisfies (the kinds of include/hgx_not.h name the
// reference lines each restates), lowered by the host to terms of literals.
//
// GPU formulation, after the union's (hgx_union.hip): a lane per clause hit over the flat hit
// space the single-pass pattern pipeline left in device memory.
//   hgx_not_eval    -- hit e of clause c: nothing to do when c has no negation; otherwise the link's row
//        (binary search of the ascending link_atom), its offset pair, its first 8 targets into registers
//        (longer rows loop over the rest in memory), its type only when a type literal is met; then the
//        clause's program -- neighbouring lanes are hits of one clause, so the program reads are
//        wave-uniform and the branches mostly are -- and a keep flag;
//   the scan        -- pre = exclusive prefix sum of the flags over the flat space (rocPRIM, sized from the
//        workspace capacity: the hit total is known on the device only);
//   hgx_not_compact -- a kept hit e goes to pre[e]; clause c's new run starts at pre[run_off[c]].  The runs
//        stay ascending and contiguous per query: the layout hgx_union_keep / hgx_union_place read.
// Both kernels read the hit total and the overflow flag of the clause stage from device memory and do nothing
// after an overflow, so no host round trip sits between the clause stage, the filter and the union; the
// host's re-run after a workspace overflow enqueues the filter again with the clause stage.
#include <rocprim/device/device_scan.hpp>

#include "hgx_not_dev.h"

namespace hgx {

namespace {

constexpr int kNotMaxOperands = 64;      // operands of one ordered / link literal
constexpr int kNotMaxTypes = 1 << 16;    // operands of one type literal

__global__ void __launch_bounds__(256) hgx_not_eval(NotArgs a) {
    if (a.stat[2]) return;   // the clause stage overflowed its workspace: the host grows it and runs again
    const int64_t H = a.run_off[a.n_clauses];
    u64 tested = 0, rejected = 0, targets_read = 0, types_read = 0, probes = 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < H; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = upper_bound_off(a.run_off, (int64_t)a.n_clauses + 1, e) - 1;
        const int64_t g0 = a.prog.neg_off[c], g1 = a.prog.neg_off[c + 1];
        if (g0 == g1) {
            a.flag[e] = 1;
            continue;
        }
        ++tested;
        const int32_t x = a.hits[e];
        int64_t row = 0, hi = a.M;   // the link's row: first row with link_atom >= x
        while (row < hi) {
            const int64_t mid = (row + hi) >> 1;
            ++probes;
            if (a.link_atom[mid] < x) row = mid + 1;
            else hi = mid;
        }
        bool keep = row < a.M && a.link_atom[row] == x;   // (a clause hit is a link atom)
        if (keep) {
            const int64_t b = a.tgt_off[row];
            Link L;
            L.tg = a.tgt_idx + b;
            L.n = (int32_t)(a.tgt_off[row + 1] - b);
#pragma unroll
            for (int k = 0; k < 8; ++k) L.r[k] = k < L.n ? L.tg[k] : -1;
            targets_read += (u64)L.n;
            int32_t type = INT32_MIN;
            keep = negations_keep(a.prog, g0, g1, L, a.link_type, row, type, types_read);
        }
        if (!keep) ++rejected;
        a.flag[e] = keep ? 1 : 0;
    }
    wave_add(a.ctr + 0, tested);
    wave_add(a.ctr + 1, rejected);
    wave_add(a.ctr + 2, targets_read);
    wave_add(a.ctr + 3, types_read);
    wave_add(a.ctr + 4, probes);
}

__global__ void __launch_bounds__(256) hgx_not_compact(NotArgs a) {
    if (a.stat[2]) return;
    const int64_t H = a.run_off[a.n_clauses];
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, ts = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = t0; e < H; e += ts)
        if (a.flag[e]) a.hits_out[a.pre[e]] = a.hits[e];
    for (int64_t c = t0; c <= a.n_clauses; c += ts) a.run_out[c] = a.pre[a.run_off[c]];
    if (t0 < 8) a.out_ctr[t0] = a.ctr[t0];
}

std::string where(int32_t n_queries, const int64_t* clause_off, int64_t c, int64_t g_in_clause) {
    const int64_t q = std::upper_bound(clause_off, clause_off + n_queries + 1, c) - clause_off - 1;
    return "hgx_pattern_batch_dnf_not: query " + std::to_string(q) + " clause " + std::to_string(c - clause_off[q]) +
           " negation " + std::to_string(g_in_clause);
}

}  // namespace

int not_check_literal(int64_t A, const NotProgram& p, int64_t l, std::string& why) {
    const int32_t kind = p.lit[4 * l], b = p.lit[4 * l + 2], e = p.lit[4 * l + 3];
    if (b < 0 || e < b || e > p.n_ops) return why = ": operand range outside ops", HGX_E_INVALID;
    const int32_t m = e - b;
    const int32_t* op = p.ops + b;
    auto bad_atom = [&](int32_t h) { return h < 0 || h >= A; };
    const char* const range = ": atom id out of range";
    const char* const limits = " exceeds the condition limits";
    switch (kind) {
    case HGX_NOT_TYPE:
        if (m > kNotMaxTypes) return why = limits, HGX_E_UNSUPPORTED;
        for (int32_t i = 0; i < m; ++i)
            if (op[i] < 0) return why = ": bad type", HGX_E_INVALID;
        break;
    case HGX_NOT_INCIDENT:
        if (m != 1) return why = ": an incident literal has one operand", HGX_E_INVALID;
        if (bad_atom(op[0])) return why = range, HGX_E_INVALID;
        break;
    case HGX_NOT_POSITIONED:
        if (m != 4) return why = ": a positioned literal has four operands", HGX_E_INVALID;
        if (bad_atom(op[0])) return why = range, HGX_E_INVALID;
        break;
    case HGX_NOT_ORDERED:
        if (m > kNotMaxOperands) return why = limits, HGX_E_UNSUPPORTED;
        for (int32_t i = 0; i < m; ++i)
            if (op[i] != HGX_ANY_HANDLE && bad_atom(op[i])) return why = range, HGX_E_INVALID;
        break;
    case HGX_NOT_LINK:
        if (m > kNotMaxOperands) return why = limits, HGX_E_UNSUPPORTED;
        for (int32_t i = 0; i < m; ++i) {
            if (op[i] != HGX_ANY_HANDLE && bad_atom(op[i])) return why = range, HGX_E_INVALID;
            for (int32_t k = 0; k < i; ++k)
                if (op[k] == op[i]) return why = ": a link set repeats a member", HGX_E_INVALID;
        }
        break;
    case HGX_NOT_ARITY:
        if (m != 1 || op[0] < 0) return why = ": bad arity literal", HGX_E_INVALID;
        break;
    default:
        return why = ": unknown literal kind " + std::to_string(kind), HGX_E_INVALID;
    }
    return HGX_OK;
}

void not_validate(int64_t A, int32_t n_queries, const int64_t* clause_off, NotProgram& p) {
    const char* who = "hgx_pattern_batch_dnf_not: ";
    const int64_t nc = clause_off[n_queries];
    // the clause and the negation inside it of negation g (neg_off checked)
    auto at_neg = [&](int64_t g) {
        const int64_t c = std::upper_bound(p.neg_off, p.neg_off + nc + 1, g) - p.neg_off - 1;
        return where(n_queries, clause_off, c, g - p.neg_off[c]);
    };
    if (p.neg_off[0] != 0) fail(HGX_E_INVALID, std::string(who) + "neg_off[0] is not 0");
    for (int64_t c = 0; c < nc; ++c)
        if (p.neg_off[c + 1] < p.neg_off[c])
            fail(HGX_E_INVALID, where(n_queries, clause_off, c, 0) + ": neg_off decreases");
    p.n_negs = p.neg_off[nc];
    if (p.n_negs == 0) return;
    if (!p.term_off) fail(HGX_E_INVALID, std::string(who) + "null term_off");
    if (p.term_off[0] != 0) fail(HGX_E_INVALID, std::string(who) + "term_off[0] is not 0");
    for (int64_t g = 0; g < p.n_negs; ++g)
        if (p.term_off[g + 1] < p.term_off[g]) fail(HGX_E_INVALID, at_neg(g) + ": term_off decreases");
    p.n_terms = p.term_off[p.n_negs];
    if (p.n_terms > 0) {
        if (!p.lit_off) fail(HGX_E_INVALID, std::string(who) + "null lit_off");
        if (p.lit_off[0] != 0) fail(HGX_E_INVALID, std::string(who) + "lit_off[0] is not 0");
        for (int64_t t = 0; t < p.n_terms; ++t)
            if (p.lit_off[t + 1] < p.lit_off[t])
                fail(HGX_E_INVALID, at_neg(std::upper_bound(p.term_off, p.term_off + p.n_negs + 1, t) - p.term_off - 1) +
                                        ": lit_off decreases");
        p.n_lits = p.lit_off[p.n_terms];
    }
    if (p.n_negs > INT32_MAX || p.n_terms > INT32_MAX || p.n_lits > INT32_MAX)
        fail(HGX_E_UNSUPPORTED, std::string(who) + "negation program too large");
    if (p.n_lits > 0 && !p.lit) fail(HGX_E_INVALID, std::string(who) + "null lit");
    if (p.n_ops < 0 || p.n_ops > INT32_MAX || (p.n_ops > 0 && !p.ops))
        fail(HGX_E_INVALID, std::string(who) + "bad ops");
    for (int64_t c = 0; c < nc; ++c)
        for (int64_t g = p.neg_off[c]; g < p.neg_off[c + 1]; ++g)
            for (int64_t t = p.term_off[g]; t < p.term_off[g + 1]; ++t)
                for (int64_t l = p.lit_off[t]; l < p.lit_off[t + 1]; ++l) {
                    std::string why;
                    if (const int rc = not_check_literal(A, p, l, why))
                        fail(rc, where(n_queries, clause_off, c, g - p.neg_off[c]) + why);
                }
}

void not_launch(const NotArgs& a, hipStream_t s) {
    const int grid = grid_for(a.cap, 256, 4096);
    HGX_HIP(hipMemsetAsync(a.ctr, 0, sizeof(u64) * 8, s));
    hgx_not_eval<<<grid, 256, 0, s>>>(a);
    HGX_CHECK_LAUNCH();
    size_t sb = a.tmp_bytes;
    HGX_HIP(rocprim::exclusive_scan(a.tmp, sb, (const uint8_t*)a.flag, a.pre, (int64_t)0, (size_t)a.cap + 1,
                                    rocprim::plus<int64_t>(), s));
    hgx_not_compact<<<grid, 256, 0, s>>>(a);
    HGX_CHECK_LAUNCH();
}

}  // namespace hgx
