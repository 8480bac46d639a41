// atoms_check -- the host side of include/hgx_atoms.h under AddressSanitizer + UBSan, no GPU: the validation of
// the part arrays for hgx_pattern_batch_atoms (hgx::join_validate with its flag set), of the keep table
// (hgx::atoms_keep_validate) and the argument checks of the three entry points that fail before any device work,
// on well-formed batches, on every malformed shape the header names, and on arrays allocated to their exact size
// (so an out-of-bounds read of a checker itself is caught).  TEST INFRASTRUCTURE: built by
// `make -C hypergraphdb_amd/csrc build/san/atoms_check`, run as its own executable (tests/test_atoms_sanitize.py).
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "../../hypergraphdb_amd/csrc/hgx_internal.h"

namespace {

int failures = 0;
const char* const kWho = "hgx_pattern_batch_atoms";

void expect(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "atoms_check: FAILED: %s\n", what);
        ++failures;
    }
}

// status of join_validate as hgx_pattern_batch_atoms calls it, on exact-size heap copies (0 = accepted)
int validate(const std::vector<int64_t>& part_off, const std::vector<int32_t>& part_pos, int32_t flags,
             std::string* msg = nullptr, int32_t n_queries = -2) {
    const std::vector<int64_t> off(part_off);
    const std::vector<int32_t> pos(part_pos);
    if (n_queries == -2) n_queries = (int32_t)off.size() - 1;
    try {
        hgx::join_validate(n_queries, off.empty() ? nullptr : off.data(), pos.empty() ? nullptr : pos.data(), flags, kWho,
                           HGX_ATOMS_TYPE_SCAN);
    } catch (const hgx::Error& e) {
        if (msg) *msg = e.msg;
        return e.code;
    }
    return 0;
}

// status of atoms_keep_validate on an exact-size copy of the table; n = the queries it counted
int keep_validate(const hgx_graph* g, const std::vector<hgx_atom_predicate*>& keep, int64_t* n, std::string* msg) {
    const std::vector<hgx_atom_predicate*> k(keep);
    try {
        *n = hgx::atoms_keep_validate(g, (int32_t)k.size(), k.data());
    } catch (const hgx::Error& e) {
        if (msg) *msg = e.msg;
        return e.code;
    }
    return 0;
}

}  // namespace

int main() {
    std::string msg;
    // --- the part arrays: three join queries with two parts, none, three parts
    const std::vector<int64_t> off = {0, 2, 2, 5};
    const std::vector<int32_t> pos = {0, HGX_JOIN_SELF, 3, 0, 1 << 20};
    expect(validate(off, pos, 0, &msg) == 0, "the well-formed arrays are accepted");
    expect(validate(off, pos, HGX_ATOMS_TYPE_SCAN, &msg) == 0, "... with the scan flag");
    expect(validate({0}, {}, 0, &msg) == 0, "a batch of 0 queries");
    expect(validate({0, 0, 0}, {}, HGX_ATOMS_TYPE_SCAN, &msg) == 0, "queries without parts: part_pos is never read");
    struct Case {
        const char* what;
        int code;
        const char* names;
        std::vector<int64_t> off;
        std::vector<int32_t> pos;
        int32_t flags;
    };
    const Case cases[] = {
        {"part_off not starting at 0", HGX_E_INVALID, "part_off[0]", {1, 2, 2, 5}, pos, 0},
        {"part_off decreasing", HGX_E_INVALID, "decreases at join query 1", {0, 2, 1, 5}, pos, 0},
        {"part_off decreasing at the end", HGX_E_INVALID, "decreases at join query 2", {0, 2, 2, 1}, pos, 0},
        {"part_pos missing", HGX_E_INVALID, "null part_pos", off, {}, 0},
        {"a position below HGX_JOIN_SELF", HGX_E_INVALID, "join query 0 part 1", off, {0, -2, 3, 0, 1}, 0},
        {"... in the last part", HGX_E_INVALID, "join query 2 part 2", off, {0, -1, 3, 0, INT32_MIN}, 0},
        {"an unknown flag", HGX_E_INVALID, "unknown flag", off, pos, 2},
        {"an unknown flag next to the known one", HGX_E_INVALID, "unknown flag", off, pos, HGX_ATOMS_TYPE_SCAN | 4},
        {"a negative flag", HGX_E_INVALID, "unknown flag", off, pos, -1},
    };
    for (const Case& c : cases) {
        msg.clear();
        const int rc = validate(c.off, c.pos, c.flags, &msg);
        const bool ok = rc == c.code && msg.find(c.names) != std::string::npos && msg.find(kWho) == 0;
        if (!ok) std::fprintf(stderr, "atoms_check: %s: status %d, message \"%s\"\n", c.what, rc, msg.c_str());
        expect(ok, c.what);
    }
    expect(validate({}, {}, 0, &msg) == HGX_E_INVALID, "a null part_off");
    expect(validate({0}, {}, 0, &msg, -1) == HGX_E_INVALID, "a negative query count");
    expect(validate({0, (int64_t)INT32_MAX - 1}, {}, 0, &msg) == HGX_E_UNSUPPORTED, "too many parts");

    // --- the keep table: host-side stand-ins (no device is touched by the checks)
    auto snap = std::make_unique<hgx_graph>(), other = std::make_unique<hgx_graph>(), ctx = std::make_unique<hgx_graph>();
    ctx->base = snap.get();
    hgx_atom_predicate mine, theirs;
    mine.root = snap.get();
    theirs.root = other.get();
    int64_t n = -1;
    expect(keep_validate(snap.get(), {&mine, nullptr, &mine}, &n, &msg) == 0 && n == 2, "one predicate serves many queries");
    expect(keep_validate(ctx.get(), {nullptr, &mine}, &n, &msg) == 0 && n == 1, "a context takes its snapshot's predicates");
    expect(keep_validate(snap.get(), {nullptr, nullptr}, &n, &msg) == 0 && n == 0, "a table of nulls");
    expect(keep_validate(snap.get(), {}, &n, &msg) == 0 && n == 0, "an empty table");
    msg.clear();
    expect(keep_validate(snap.get(), {&mine, nullptr, &theirs}, &n, &msg) == HGX_E_INVALID &&
               msg.find("join query 2") != std::string::npos && msg.find("another graph") != std::string::npos,
           "a predicate of another graph names its join query");
    msg.clear();
    expect(keep_validate(ctx.get(), {&theirs}, &n, &msg) == HGX_E_INVALID && msg.find("join query 0") != std::string::npos,
           "... on a context too");
    expect(keep_validate(other.get(), {&mine}, &n, &msg) == HGX_E_INVALID, "... and the other way round");

    // --- the entry points: what fails before any device work
    hgx_query_result* r = (hgx_query_result*)1;
    const int64_t off1[2] = {0, 1}, zero[1] = {0};
    const int32_t pos1[1] = {0};
    expect(hgx_pattern_batch_atoms(nullptr, 0, zero, nullptr, nullptr, zero, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   0, 0, &r) == HGX_E_INVALID, "a null graph");
    expect(hgx_pattern_batch_atoms(snap.get(), 0, zero, nullptr, nullptr, zero, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   0, 0, nullptr) == HGX_E_INVALID, "a null out");
    r = (hgx_query_result*)1;
    expect(hgx_pattern_batch_atoms(snap.get(), 1, off1, pos1, nullptr, zero, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   0, 2, &r) == HGX_E_INVALID && r == nullptr &&
               std::string(hgx_last_error()).find("unknown flag") != std::string::npos,
           "an unknown flag through the ABI clears out");
    hgx_atom_predicate* const bad[1] = {&theirs};
    expect(hgx_pattern_batch_atoms(snap.get(), 1, off1, pos1, bad, zero, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   0, 0, &r) == HGX_E_INVALID &&
               std::string(hgx_last_error()).find("join query 0") != std::string::npos,
           "a foreign predicate through the ABI");
    {   // a partition shard is refused by both entry points
        auto shard = std::make_unique<hgx_graph>();
        hgx::ShardInfo info;
        shard->shard = &info;
        int64_t cnt = 0;
        const int32_t t = 0;
        expect(hgx_pattern_batch_atoms(shard.get(), 1, off1, pos1, nullptr, zero, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr, 0, HGX_ATOMS_TYPE_SCAN, &r) == HGX_E_UNSUPPORTED, "a shard: the batch");
        expect(hgx_graph_type_atoms(shard.get(), &t, 1, &cnt) == HGX_E_UNSUPPORTED, "a shard: the histogram");
        shard->shard = nullptr;
    }
    {
        int64_t cnt = 0;
        const int32_t t = 0;
        expect(hgx_graph_type_atoms(nullptr, &t, 1, &cnt) == HGX_E_INVALID, "type_atoms: a null graph");
        expect(hgx_graph_type_atoms(snap.get(), nullptr, 1, &cnt) == HGX_E_INVALID, "type_atoms: null types");
        expect(hgx_graph_type_atoms(snap.get(), &t, 1, nullptr) == HGX_E_INVALID, "type_atoms: null counts");
        expect(hgx_graph_type_atoms(snap.get(), &t, -1, &cnt) == HGX_E_INVALID, "type_atoms: a negative count");
    }
    expect(hgx_query_result_atoms_stats(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == HGX_E_INVALID,
           "atoms_stats: a null result");
    if (failures) return 1;
    std::printf("atoms_check: all checks passed\n");
    return 0;
}
