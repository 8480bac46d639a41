// not_check -- the host side of hgx_pattern_batch_dnf_not under AddressSanitizer + UBSan, no GPU: the
// validation of the negation program (hgx::not_validate, hgx_not.hip) on well-formed programs, on every
// malformed shape it names in include/hgx_not.h, and on truncated arrays allocated to their exact size (so an
// out-of-bounds read of the checker itself is caught).  TEST INFRASTRUCTURE: built by
// `make -C hypergraphdb_amd/csrc build/san/not_check`, run as its own executable (tests/test_not_sanitize.py).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../hypergraphdb_amd/csrc/hgx_internal.h"

namespace {

int failures = 0;

struct Prog {
    std::vector<int64_t> neg_off, term_off, lit_off;
    std::vector<int32_t> lit, ops;
};

// status of not_validate on exact-size heap copies of the arrays (0 = accepted); msg = its message
int validate(int64_t A, const std::vector<int64_t>& clause_off, const Prog& p, std::string* msg = nullptr,
             hgx::NotProgram* out = nullptr) {
    hgx::NotProgram np;
    np.neg_off = p.neg_off.data();
    np.term_off = p.term_off.empty() ? nullptr : p.term_off.data();
    np.lit_off = p.lit_off.empty() ? nullptr : p.lit_off.data();
    np.lit = p.lit.empty() ? nullptr : p.lit.data();
    np.ops = p.ops.empty() ? nullptr : p.ops.data();
    np.n_ops = (int64_t)p.ops.size();
    try {
        hgx::not_validate(A, (int32_t)clause_off.size() - 1, clause_off.data(), np);
    } catch (const hgx::Error& e) {
        if (msg) *msg = e.msg;
        return e.code;
    }
    if (out) *out = np;
    return 0;
}

void expect(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "not_check: FAILED: %s\n", what);
        ++failures;
    }
}

// two queries, three clauses; clause 0: Not(incident(4) | !type{1,2}), clause 1: none,
// clause 2: Not(orderedLink(7, ANY, 8) & link{9, 10} & arity 2), Not(incidentNotAt(5, -2, 3)), Not(Or()), Not(And())
Prog good() {
    Prog p;
    p.neg_off = {0, 1, 1, 5};
    p.term_off = {0, 2, 3, 4, 4, 5};
    p.lit_off = {0, 1, 2, 5, 6, 6};
    p.lit = {HGX_NOT_INCIDENT, 1, 0, 1, HGX_NOT_TYPE, 0, 1, 3, HGX_NOT_ORDERED, 1, 3, 6, HGX_NOT_LINK, 1, 6, 8,
             HGX_NOT_ARITY, 1, 8, 9, HGX_NOT_POSITIONED, 1, 9, 13};
    p.ops = {4, 1, 2, 7, HGX_ANY_HANDLE, 8, 9, 10, 2, 5, -2, 3, 1};
    return p;
}

}  // namespace

int main() {
    const std::vector<int64_t> clause_off = {0, 1, 3};
    const int64_t A = 11;
    std::string msg;
    hgx::NotProgram np;
    expect(validate(A, clause_off, good(), &msg, &np) == 0, "the well-formed program is accepted");
    expect(np.n_negs == 5 && np.n_terms == 5 && np.n_lits == 6, "its totals");
    {   // no negation at all: nothing else is read
        Prog p;
        p.neg_off = {0, 0, 0, 0};
        expect(validate(A, clause_off, p, &msg, &np) == 0 && np.n_negs == 0, "a program without negations");
    }
    {   // negations without terms: lit_off, lit and ops may be absent
        Prog p;
        p.neg_off = {0, 1, 1, 2};
        p.term_off = {0, 0, 0};
        expect(validate(A, clause_off, p, &msg, &np) == 0 && np.n_terms == 0, "negations without terms");
    }
    struct Case {
        const char* what;
        int code;
        const char* names;
        void (*edit)(Prog&);
    };
    const Case cases[] = {
        {"neg_off not starting at 0", HGX_E_INVALID, "neg_off", [](Prog& p) { p.neg_off[0] = 1; }},
        {"neg_off decreasing", HGX_E_INVALID, "query 1 clause 0", [](Prog& p) { p.neg_off[1] = 2; }},
        {"term_off missing", HGX_E_INVALID, "term_off", [](Prog& p) { p.term_off.clear(); }},
        {"term_off not starting at 0", HGX_E_INVALID, "term_off", [](Prog& p) { p.term_off[0] = 1; }},
        {"term_off decreasing", HGX_E_INVALID, "query 1 clause 1 negation 0", [](Prog& p) { p.term_off[2] = 1; }},
        {"lit_off missing", HGX_E_INVALID, "lit_off", [](Prog& p) { p.lit_off.clear(); }},
        {"lit_off decreasing", HGX_E_INVALID, "query 1 clause 1 negation 0", [](Prog& p) { p.lit_off[3] = 1; }},
        {"lit missing", HGX_E_INVALID, "lit", [](Prog& p) { p.lit.clear(); }},
        {"ops missing", HGX_E_INVALID, "ops", [](Prog& p) { p.ops.clear(); }},
        {"operand range past ops", HGX_E_INVALID, "query 1 clause 1 negation 1", [](Prog& p) { p.lit[4 * 5 + 3] = 14; }},
        {"operand range reversed", HGX_E_INVALID, "query 0 clause 0 negation 0", [](Prog& p) { p.lit[2] = 2; }},
        {"negative operand offset", HGX_E_INVALID, "negation", [](Prog& p) { p.lit[2] = -1; }},
        {"unknown kind", HGX_E_INVALID, "unknown literal kind 9", [](Prog& p) { p.lit[4] = 9; }},
        {"kind 0", HGX_E_INVALID, "unknown literal kind 0", [](Prog& p) { p.lit[0] = 0; }},
        {"incident id out of range", HGX_E_INVALID, "query 0 clause 0 negation 0", [](Prog& p) { p.ops[0] = 11; }},
        {"negative incident id", HGX_E_INVALID, "atom id out of range", [](Prog& p) { p.ops[0] = -1; }},
        {"pattern id out of range", HGX_E_INVALID, "query 1 clause 1 negation 0", [](Prog& p) { p.ops[5] = 99; }},
        {"link member out of range", HGX_E_INVALID, "atom id out of range", [](Prog& p) { p.ops[7] = 11; }},
        {"link set repeats a member", HGX_E_INVALID, "repeats", [](Prog& p) { p.ops[7] = 9; }},
        {"positioned target out of range", HGX_E_INVALID, "query 1 clause 1 negation 1", [](Prog& p) { p.ops[9] = 50; }},
        {"positioned record too short", HGX_E_INVALID, "four operands", [](Prog& p) { p.lit[4 * 5 + 2] = 10; }},
        {"incident with two operands", HGX_E_INVALID, "one operand", [](Prog& p) { p.lit[3] = 2; }},
        {"negative arity", HGX_E_INVALID, "arity", [](Prog& p) { p.ops[8] = -3; }},
        {"negative type", HGX_E_INVALID, "bad type", [](Prog& p) { p.ops[2] = -1; }},
    };
    for (const Case& c : cases) {
        Prog p = good();
        c.edit(p);
        msg.clear();
        const int rc = validate(A, clause_off, p, &msg);
        const bool ok = rc == c.code && msg.find(c.names) != std::string::npos;
        if (!ok) std::fprintf(stderr, "not_check: %s: status %d, message \"%s\"\n", c.what, rc, msg.c_str());
        expect(ok, c.what);
    }
    {   // the limits: 64 operands of a pattern or a link set pass, 65 are HGX_E_UNSUPPORTED
        for (int kind : {HGX_NOT_ORDERED, HGX_NOT_LINK})
            for (int m : {64, 65}) {
                Prog p;
                p.neg_off = {0, 1, 1, 1};
                p.term_off = {0, 1};
                p.lit_off = {0, 1};
                p.lit = {kind, 1, 0, m};
                for (int i = 0; i < m; ++i) p.ops.push_back(kind == HGX_NOT_LINK ? i : 3);
                const int rc = validate(100, clause_off, p, &msg);
                expect(rc == (m == 64 ? 0 : HGX_E_UNSUPPORTED), "the operand limit of a pattern / a link set");
            }
    }
    if (failures) return 1;
    std::printf("not_check: all checks passed\n");
    return 0;
}
