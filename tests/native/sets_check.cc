// sets_check -- the host side of hgx_bfs_result_sets under AddressSanitizer + UBSan, no GPU: the argument checks
// (hgx::sets_validate, hgx_sets.hip) on well-formed selections, on every refusal of include/hgx_sets.h that is
// decided without a device, and on seed-index arrays allocated to their exact size (so an out-of-bounds read of the
// checker itself is caught); then the null-argument refusals of the entry points themselves.  TEST INFRASTRUCTURE:
// built by `make -C hypergraphdb_amd/csrc build/san/sets_check`, run as its own executable
// (tests/test_sets_sanitize.py).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../hypergraphdb_amd/csrc/hgx_internal.h"

namespace {

int failures = 0;

struct Call {
    bool have_result = true, have_out = true, shard = false;
    int32_t n_result_seeds = 100;
    std::vector<int32_t> idx;        // copied to a heap array of its exact size
    int32_t n_sets = -2;             // -2: idx.size()
    bool null_idx = false;
    int32_t min_depth = 0, max_depth = HGX_UNBOUNDED;
    uint32_t flags = 0;
};

// status of sets_validate (0 = accepted); msg = its message
int validate(const Call& c, std::string* msg = nullptr) {
    const std::vector<int32_t> exact(c.idx);   // exactly idx.size() elements on the heap
    try {
        hgx::sets_validate(c.have_result, c.have_out, c.shard, c.n_result_seeds,
                           c.null_idx || exact.empty() ? nullptr : exact.data(),
                           c.n_sets == -2 ? (int32_t)exact.size() : c.n_sets, c.min_depth, c.max_depth, c.flags);
    } catch (const hgx::Error& e) {
        if (msg) *msg = e.msg;
        return e.code;
    }
    return 0;
}

void expect(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "sets_check: FAILED: %s\n", what);
        ++failures;
    }
}

Call good() {
    Call c;
    c.idx = {5, 0, 99, 64, 63};
    return c;
}

}  // namespace

int main() {
    std::string msg;
    expect(validate(good(), &msg) == 0, "a well-formed selection in non-monotone order is accepted");
    {
        Call c;
        expect(validate(c) == 0, "an empty selection needs no seed_index");
        c.idx = {7};
        c.n_sets = 0;
        expect(validate(c) == 0, "n_sets 0 reads nothing of seed_index");
    }
    {
        Call c = good();
        c.min_depth = 3;
        c.max_depth = 3;
        c.flags = HGX_SETS_DEPTHS | HGX_SETS_COUNT_ONLY;
        expect(validate(c) == 0, "min_depth == max_depth and both flags");
        c.max_depth = HGX_UNBOUNDED;
        expect(validate(c) == 0, "an unbounded range above a positive min_depth");
    }
    {   // every seed of the result, once
        Call c;
        for (int32_t i = 0; i < c.n_result_seeds; ++i) c.idx.push_back(c.n_result_seeds - 1 - i);
        expect(validate(c) == 0, "every seed in reverse order");
    }
    struct Case {
        const char* what;
        int code;
        const char* names;
        void (*edit)(Call&);
    };
    const Case cases[] = {
        {"null result", HGX_E_INVALID, "null result", [](Call& c) { c.have_result = false; }},
        {"null out", HGX_E_INVALID, "null out", [](Call& c) { c.have_out = false; }},
        {"negative n_sets", HGX_E_INVALID, "n_sets -1", [](Call& c) { c.n_sets = -1; }},
        {"negative min_depth", HGX_E_INVALID, "min_depth -1", [](Call& c) { c.min_depth = -1; }},
        {"max_depth below min_depth", HGX_E_INVALID, "max_depth 1 is below min_depth 2",
         [](Call& c) { c.min_depth = 2; c.max_depth = 1; }},
        {"a negative max_depth that is not HGX_UNBOUNDED", HGX_E_INVALID, "max_depth -2",
         [](Call& c) { c.max_depth = -2; }},
        {"unknown flag bits", HGX_E_INVALID, "unknown flag bits 4", [](Call& c) { c.flags = 4; }},
        {"unknown flag bits next to known ones", HGX_E_INVALID, "unknown flag bits",
         [](Call& c) { c.flags = HGX_SETS_DEPTHS | 0x80000000u; }},
        {"a shard result", HGX_E_UNSUPPORTED, "partition shard", [](Call& c) { c.shard = true; }},
        {"null seed_index", HGX_E_INVALID, "null seed_index", [](Call& c) { c.null_idx = true; c.n_sets = 5; }},
        {"a seed index past the result", HGX_E_NOTFOUND, "set 2: no such seed index 100", [](Call& c) { c.idx[2] = 100; }},
        {"a negative seed index", HGX_E_NOTFOUND, "set 0: no such seed index -1", [](Call& c) { c.idx[0] = -1; }},
        {"the last entry is checked too", HGX_E_NOTFOUND, "set 4: no such seed index 1000", [](Call& c) { c.idx[4] = 1000; }},
        {"a repeated seed index", HGX_E_INVALID, "set 4: seed index 0 repeats set 1", [](Call& c) { c.idx[4] = 0; }},
        {"a seed index repeated at once", HGX_E_INVALID, "set 1: seed index 5 repeats set 0", [](Call& c) { c.idx[1] = 5; }},
    };
    for (const Case& c : cases) {
        Call k = good();
        c.edit(k);
        msg.clear();
        const int rc = validate(k, &msg);
        const bool ok = rc == c.code && msg.find(c.names) != std::string::npos &&
                        msg.find("hgx_bfs_result_sets") != std::string::npos;
        if (!ok) std::fprintf(stderr, "sets_check: %s: status %d, message \"%s\"\n", c.what, rc, msg.c_str());
        expect(ok, c.what);
    }
    {   // a result without seeds: every index is outside it
        Call c;
        c.n_result_seeds = 0;
        c.idx = {0};
        expect(validate(c) == HGX_E_NOTFOUND, "a result without seeds");
    }

    // the entry points themselves: what they refuse without a result or an object
    hgx_visited_sets* vs = nullptr;
    const int32_t one[1] = {0};
    expect(hgx_bfs_result_sets(nullptr, one, 1, 0, HGX_UNBOUNDED, nullptr, 0, -1, &vs) == HGX_E_INVALID && !vs,
           "hgx_bfs_result_sets without a result");
    expect(std::strstr(hgx_last_error(), "null result") != nullptr, "its message");
    int32_t n = 0;
    int64_t tot = 0, off[1];
    uint32_t fl = 0;
    double ms = 0, by = 0;
    expect(hgx_visited_sets_info(nullptr, &n, &tot, &fl) == HGX_E_INVALID, "hgx_visited_sets_info without an object");
    expect(hgx_visited_sets_offsets(nullptr, off) == HGX_E_INVALID, "hgx_visited_sets_offsets without an object");
    expect(hgx_visited_sets_read(nullptr, 0, 0, nullptr, nullptr) == HGX_E_INVALID, "hgx_visited_sets_read without an object");
    expect(hgx_visited_sets_stats(nullptr, &tot, &tot, &ms, &by) == HGX_E_INVALID, "hgx_visited_sets_stats without an object");
    hgx_visited_sets_free(nullptr);
    if (failures) return 1;
    std::printf("sets_check: all checks passed\n");
    return 0;
}
