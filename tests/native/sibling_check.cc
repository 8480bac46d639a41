// sibling_check -- the host side of hgx_atom_predicate_create and hgx_graph_set_atom_types under AddressSanitizer +
// UBSan, no GPU: the validation of an atom program (hgx::atompred_validate, hgx_sibling.hip) and of an atom-type
// column (hgx::atom_types_validate) on well-formed input, on every malformed shape include/hgx_sibling.h names, and
// on arrays allocated to their exact size (so an out-of-bounds read of the checker itself is caught).  TEST
// INFRASTRUCTURE: built by `make -C hypergraphdb_amd/csrc build/san/sibling_check`, run as its own executable
// (tests/test_sibling_sanitize.py).
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

// status of atompred_validate on exact-size heap copies of the arrays (0 = accepted); msg = its message
int validate(int64_t A, const Prog& p, std::string* msg = nullptr, hgx::NotProgram* out = nullptr, int64_t n_terms = -1) {
    hgx::NotProgram np;
    np.lit_off = p.lit_off.empty() ? nullptr : p.lit_off.data();
    np.lit = p.lit.empty() ? nullptr : p.lit.data();
    np.ops = p.ops.empty() ? nullptr : p.ops.data();
    np.n_ops = (int64_t)p.ops.size();
    try {
        hgx::atompred_validate(A, n_terms >= 0 ? n_terms : p.n_terms(), np);
    } catch (const hgx::Error& e) {
        if (msg) *msg = e.msg;
        return e.code;
    }
    if (out) *out = np;
    return 0;
}

// status of atom_types_validate on exact-size copies
int types(const std::vector<int32_t>& at, const std::vector<int32_t>& la, const std::vector<int32_t>& lt,
          std::string* msg = nullptr) {
    try {
        hgx::atom_types_validate((int64_t)at.size(), (int64_t)la.size(), at.empty() ? nullptr : at.data(),
                                 la.empty() ? nullptr : la.data(), lt.empty() ? nullptr : lt.data());
    } catch (const hgx::Error& e) {
        if (msg) *msg = e.msg;
        return e.code;
    }
    return 0;
}

void expect(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "sibling_check: FAILED: %s\n", what);
        ++failures;
    }
}

// (typePlus{0, 1, 2} & !type 1) | (type 4 & typePlus{4, 5}) | !typePlus{1, 3}
Prog good() {
    Prog p;
    p.lit_off = {0, 2, 4, 5};
    p.lit = {HGX_NOT_TYPE, 1, 0, 3, HGX_NOT_TYPE, 0, 3, 4, HGX_NOT_TYPE, 1, 4, 5, HGX_NOT_TYPE, 1, 5, 7,
             HGX_NOT_TYPE, 0, 7, 9};
    p.ops = {0, 1, 2, 1, 4, 4, 5, 1, 3};
    return p;
}

}  // namespace

int main() {
    const int64_t A = 11;
    std::string msg;
    hgx::NotProgram np;
    expect(validate(A, good(), &msg, &np) == 0, "the well-formed program is accepted");
    expect(np.n_terms == 3 && np.n_lits == 5, "its totals");
    {   // the empty Or: no term, every array may be absent
        Prog p;
        expect(validate(A, p, &msg, &np) == 0 && np.n_terms == 0 && np.n_lits == 0, "a predicate without terms");
    }
    {   // the empty And: one term without literals, lit and ops may be absent
        Prog p;
        p.lit_off = {0, 0};
        expect(validate(A, p, &msg, &np) == 0 && np.n_terms == 1 && np.n_lits == 0, "a predicate of one empty term");
    }
    {   // a type literal without operands (typePlus of nothing) reads no operand
        Prog p;
        p.lit_off = {0, 1};
        p.lit = {HGX_NOT_TYPE, 0, 1, 1};
        p.ops = {5};
        expect(validate(A, p, &msg, &np) == 0 && np.n_lits == 1, "an empty type set");
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
        {"lit_off decreasing", HGX_E_INVALID, "term 1: lit_off decreases", [](Prog& p) { p.lit_off[2] = 1; }},
        {"lit missing", HGX_E_INVALID, "null lit", [](Prog& p) { p.lit.clear(); }},
        {"ops missing", HGX_E_INVALID, "ops", [](Prog& p) { p.ops.clear(); }},
        {"operand range past ops", HGX_E_INVALID, "term 2 literal 0: operand range", [](Prog& p) { p.lit[4 * 4 + 3] = 10; }},
        {"operand range reversed", HGX_E_INVALID, "term 0 literal 0: operand range", [](Prog& p) { p.lit[2] = 4; }},
        {"negative operand offset", HGX_E_INVALID, "operand range", [](Prog& p) { p.lit[2] = -1; }},
        {"unknown kind", HGX_E_INVALID, "term 0 literal 1: unknown literal kind 9", [](Prog& p) { p.lit[4] = 9; }},
        {"kind 0", HGX_E_INVALID, "unknown literal kind 0", [](Prog& p) { p.lit[0] = 0; }},
        {"negative type", HGX_E_INVALID, "bad type", [](Prog& p) { p.ops[2] = -1; }},
        {"an arity literal", HGX_E_UNSUPPORTED, "term 0 literal 1: only type literals",
         [](Prog& p) { p.lit[4] = HGX_NOT_ARITY; }},
        {"an incident literal", HGX_E_UNSUPPORTED, "term 0 literal 1: only type literals",
         [](Prog& p) { p.lit[4] = HGX_NOT_INCIDENT; }},
        {"a link literal", HGX_E_UNSUPPORTED, "term 1 literal 1: only type literals",
         [](Prog& p) { p.lit[4 * 3] = HGX_NOT_LINK; }},
        {"an incident literal whose atom is out of range", HGX_E_INVALID, "atom id out of range",
         [](Prog& p) { p.lit[4] = HGX_NOT_INCIDENT; p.ops[3] = 11; }},
    };
    for (const Case& c : cases) {
        Prog p = good();
        c.edit(p);
        msg.clear();
        const int rc = validate(A, p, &msg, nullptr, 3);
        const bool ok = rc == c.code && msg.find(c.names) != std::string::npos &&
                        msg.find("hgx_atom_predicate_create") != std::string::npos;
        if (!ok) std::fprintf(stderr, "sibling_check: %s: status %d, message \"%s\"\n", c.what, rc, msg.c_str());
        expect(ok, c.what);
    }
    expect(validate(A, good(), &msg, nullptr, 0) == 0, "n_terms 0 reads nothing of the arrays");
    {
        hgx::NotProgram bad;
        int rc = 0;
        try {
            hgx::atompred_validate(A, -1, bad);
        } catch (const hgx::Error& e) {
            rc = e.code;
        }
        expect(rc == HGX_E_INVALID, "a negative term count");
    }
    for (int over : {0, 1}) {   // the limit of a type set: 65536 pass, 65537 are HGX_E_UNSUPPORTED
        const int m = 65536 + over;
        Prog p;
        p.lit_off = {0, 1};
        p.lit = {HGX_NOT_TYPE, 1, 0, m};
        for (int i = 0; i < m; ++i) p.ops.push_back(i);
        const int rc = validate(A, p, &msg);
        expect(rc == (over ? HGX_E_UNSUPPORTED : 0), "the operand limit of a type set");
        if (over) expect(msg.find("term 0 literal 0") != std::string::npos, "the limit's message names the literal");
    }

    // the atom-type column: atoms 0..5, link rows at atoms 2 (type 7), 4 (no type) and 5 (type 0)
    const std::vector<int32_t> la = {2, 4, 5}, lt = {7, -1, 0};
    expect(types({1, 1, 7, 3, 9, 0}, la, lt) == 0, "a column that agrees with the link types");
    expect(types({}, {}, {}) == 0, "an empty graph");
    expect(types({3, 4}, {}, {}) == 0, "a graph without links");
    expect(types({1, 1, 7, 3, -9, 0}, la, lt, &msg) == HGX_E_INVALID && msg.find("atom 4") != std::string::npos &&
               msg.find("hgx_graph_set_atom_types") != std::string::npos,
           "a negative type, named by its atom");
    expect(types({1, 1, 6, 3, 9, 0}, la, lt, &msg) == HGX_E_INVALID && msg.find("link row 0") != std::string::npos &&
               msg.find("atom 2") != std::string::npos,
           "a link atom whose type differs, named by its row");
    expect(types({1, 1, 7, 3, 9, 2}, la, lt, &msg) == HGX_E_INVALID && msg.find("link row 2") != std::string::npos,
           "the last row is checked too");
    expect(types({1, 1, 7}, {2, 9}, {7, 3}) == 0, "a shard-style row whose atom is outside the id space pins nothing");
    if (failures) return 1;
    std::printf("sibling_check: all checks passed\n");
    return 0;
}
