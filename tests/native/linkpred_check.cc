// linkpred_check -- the host side of hgx_link_predicate_create under AddressSanitizer + UBSan, no GPU: the
// validation of a link predicate (hgx::linkpred_validate, hgx_linkpred.hip) on well-formed programs, on every
// malformed shape it names in include/hgx_linkpred.h, and on arrays allocated to their exact size (so an
// out-of-bounds read of the checker itself is caught).  TEST INFRASTRUCTURE: built by
// `make -C hypergraphdb_amd/csrc build/san/linkpred_check`, run as its own executable
// (tests/test_linkpred_sanitize.py).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../hypergraphdb_amd/csrc/hgx_internal.h"

namespace {

int failures = 0;

struct Prog {
    std::vector<int64_t> lit_off;
    std::vector<int32_t> lit, ops;
    int64_t n_terms() const { return lit_off.empty() ? 0 : (int64_t)lit_off.size() - 1; }
};

// status of linkpred_validate on exact-size heap copies of the arrays (0 = accepted); msg = its message
int validate(int64_t A, const Prog& p, std::string* msg = nullptr, hgx::NotProgram* out = nullptr,
             bool* needs_targets = nullptr, int64_t n_terms = -1) {
    hgx::NotProgram np;
    np.lit_off = p.lit_off.empty() ? nullptr : p.lit_off.data();
    np.lit = p.lit.empty() ? nullptr : p.lit.data();
    np.ops = p.ops.empty() ? nullptr : p.ops.data();
    np.n_ops = (int64_t)p.ops.size();
    bool nt = false;
    try {
        hgx::linkpred_validate(A, n_terms >= 0 ? n_terms : p.n_terms(), np, &nt);
    } catch (const hgx::Error& e) {
        if (msg) *msg = e.msg;
        return e.code;
    }
    if (out) *out = np;
    if (needs_targets) *needs_targets = nt;
    return 0;
}

void expect(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "linkpred_check: FAILED: %s\n", what);
        ++failures;
    }
}

// incident(4) | !type{1,2} | (orderedLink(7, ANY, 8) & link{9, 10} & arity 2) | incidentNotAt(5, -2, 3) | And()
Prog good() {
    Prog p;
    p.lit_off = {0, 1, 2, 5, 6, 6};
    p.lit = {HGX_NOT_INCIDENT, 1, 0, 1, HGX_NOT_TYPE, 0, 1, 3, HGX_NOT_ORDERED, 1, 3, 6, HGX_NOT_LINK, 1, 6, 8,
             HGX_NOT_ARITY, 1, 8, 9, HGX_NOT_POSITIONED, 1, 9, 13};
    p.ops = {4, 1, 2, 7, HGX_ANY_HANDLE, 8, 9, 10, 2, 5, -2, 3, 1};
    return p;
}

}  // namespace

int main() {
    const int64_t A = 11;
    std::string msg;
    hgx::NotProgram np;
    bool nt = false;
    expect(validate(A, good(), &msg, &np, &nt) == 0, "the well-formed program is accepted");
    expect(np.n_terms == 5 && np.n_lits == 6 && nt, "its totals, and that it reads targets");
    {   // the empty Or: no term, every array may be absent
        Prog p;
        expect(validate(A, p, &msg, &np, &nt) == 0 && np.n_terms == 0 && np.n_lits == 0 && !nt, "a predicate without terms");
    }
    {   // the empty And: one term without literals, lit and ops may be absent
        Prog p;
        p.lit_off = {0, 0};
        expect(validate(A, p, &msg, &np, &nt) == 0 && np.n_terms == 1 && np.n_lits == 0 && !nt, "a predicate of one empty term");
    }
    {   // type and arity literals only: no target is read
        Prog p;
        p.lit_off = {0, 2, 3};
        p.lit = {HGX_NOT_TYPE, 1, 0, 2, HGX_NOT_ARITY, 0, 2, 3, HGX_NOT_TYPE, 0, 3, 3};
        p.ops = {1, 2, 3};
        expect(validate(A, p, &msg, &np, &nt) == 0 && np.n_lits == 3 && !nt, "a type / arity program reads no targets");
    }
    struct Case {
        const char* what;
        int code;
        const char* names;
        void (*edit)(Prog&);
    };
    const Case cases[] = {
        {"lit_off missing", HGX_E_INVALID, "lit_off", [](Prog& p) { p.lit_off.clear(); }},
        {"lit_off not starting at 0", HGX_E_INVALID, "lit_off[0]", [](Prog& p) { p.lit_off[0] = 1; }},
        {"lit_off decreasing", HGX_E_INVALID, "term 2: lit_off decreases", [](Prog& p) { p.lit_off[3] = 1; }},
        {"lit missing", HGX_E_INVALID, "null lit", [](Prog& p) { p.lit.clear(); }},
        {"ops missing", HGX_E_INVALID, "ops", [](Prog& p) { p.ops.clear(); }},
        {"operand range past ops", HGX_E_INVALID, "term 3 literal 0: operand range", [](Prog& p) { p.lit[4 * 5 + 3] = 14; }},
        {"operand range reversed", HGX_E_INVALID, "term 0 literal 0: operand range", [](Prog& p) { p.lit[2] = 2; }},
        {"negative operand offset", HGX_E_INVALID, "operand range", [](Prog& p) { p.lit[2] = -1; }},
        {"unknown kind", HGX_E_INVALID, "term 1 literal 0: unknown literal kind 9", [](Prog& p) { p.lit[4] = 9; }},
        {"kind 0", HGX_E_INVALID, "unknown literal kind 0", [](Prog& p) { p.lit[0] = 0; }},
        {"incident id out of range", HGX_E_INVALID, "term 0 literal 0: atom id out of range", [](Prog& p) { p.ops[0] = 11; }},
        {"negative incident id", HGX_E_INVALID, "atom id out of range", [](Prog& p) { p.ops[0] = -1; }},
        {"pattern id out of range", HGX_E_INVALID, "term 2 literal 0", [](Prog& p) { p.ops[5] = 99; }},
        {"link member out of range", HGX_E_INVALID, "term 2 literal 1: atom id out of range", [](Prog& p) { p.ops[7] = 11; }},
        {"link set repeats a member", HGX_E_INVALID, "repeats", [](Prog& p) { p.ops[7] = 9; }},
        {"positioned target out of range", HGX_E_INVALID, "term 3 literal 0", [](Prog& p) { p.ops[9] = 50; }},
        {"positioned record too short", HGX_E_INVALID, "four operands", [](Prog& p) { p.lit[4 * 5 + 2] = 10; }},
        {"incident with two operands", HGX_E_INVALID, "one operand", [](Prog& p) { p.lit[3] = 2; }},
        {"negative arity", HGX_E_INVALID, "term 2 literal 2: bad arity", [](Prog& p) { p.ops[8] = -3; }},
        {"negative type", HGX_E_INVALID, "bad type", [](Prog& p) { p.ops[2] = -1; }},
    };
    for (const Case& c : cases) {
        Prog p = good();
        c.edit(p);
        msg.clear();
        const int rc = validate(A, p, &msg, nullptr, nullptr, 5);
        const bool ok = rc == c.code && msg.find(c.names) != std::string::npos &&
                        msg.find("hgx_link_predicate_create") != std::string::npos;
        if (!ok) std::fprintf(stderr, "linkpred_check: %s: status %d, message \"%s\"\n", c.what, rc, msg.c_str());
        expect(ok, c.what);
    }
    expect(validate(A, good(), &msg, nullptr, nullptr, 0) == 0, "n_terms 0 reads nothing of the arrays");
    {
        hgx::NotProgram bad;
        bool b = false;
        int rc = 0;
        try {
            hgx::linkpred_validate(A, -1, bad, &b);
        } catch (const hgx::Error& e) {
            rc = e.code;
        }
        expect(rc == HGX_E_INVALID, "a negative term count");
    }
    {   // the limits: 64 operands of a pattern or a link set pass, 65 are HGX_E_UNSUPPORTED; 65536 / 65537 types
        for (int kind : {HGX_NOT_ORDERED, HGX_NOT_LINK, HGX_NOT_TYPE})
            for (int over : {0, 1}) {
                const int m = (kind == HGX_NOT_TYPE ? 65536 : 64) + over;
                Prog p;
                p.lit_off = {0, 1};
                p.lit = {kind, 1, 0, m};
                for (int i = 0; i < m; ++i) p.ops.push_back(kind == HGX_NOT_ORDERED ? 3 : i);
                const int rc = validate(1 << 20, p, &msg);
                expect(rc == (over ? HGX_E_UNSUPPORTED : 0), "the operand limit of a pattern / a link set / a type set");
                if (over) expect(msg.find("term 0 literal 0") != std::string::npos, "the limit's message names the literal");
            }
    }
    if (failures) return 1;
    std::printf("linkpred_check: all checks passed\n");
    return 0;
}
