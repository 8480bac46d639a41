// join_check -- the host side of hgx_pattern_batch_join under AddressSanitizer + UBSan, no GPU: the validation
// of the part arrays (hgx::join_validate, hgx_join.hip) on well-formed arrays, on every malformed shape it names
// in include/hgx_join.h, and on arrays allocated to their exact size (so an out-of-bounds read of the checker
// itself is caught); the width of the part field of the sort key (hgx::join_part_bits).  TEST INFRASTRUCTURE:
// built by `make -C hypergraphdb_amd/csrc build/san/join_check`, run as its own executable
// (tests/test_join_sanitize.py).
#include <cstdio>
#include <string>
#include <vector>

#include "../../hypergraphdb_amd/csrc/hgx_internal.h"

namespace {

int failures = 0;

// status of join_validate on exact-size heap copies of the arrays (0 = accepted); msg = its message
int validate(const std::vector<int64_t>& part_off, const std::vector<int32_t>& part_pos, int32_t flags,
             std::string* msg = nullptr, int32_t n_queries = -2) {
    const std::vector<int64_t> off(part_off);   // exact-size copies
    const std::vector<int32_t> pos(part_pos);
    if (n_queries == -2) n_queries = (int32_t)off.size() - 1;
    try {
        hgx::join_validate(n_queries, off.empty() ? nullptr : off.data(), pos.empty() ? nullptr : pos.data(), flags);
    } catch (const hgx::Error& e) {
        if (msg) *msg = e.msg;
        return e.code;
    }
    return 0;
}

void expect(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "join_check: FAILED: %s\n", what);
        ++failures;
    }
}

}  // namespace

int main() {
    std::string msg;
    // three join queries: two parts, none, three parts
    const std::vector<int64_t> off = {0, 2, 2, 5};
    const std::vector<int32_t> pos = {0, HGX_JOIN_SELF, 3, 0, 1 << 20};
    expect(validate(off, pos, 0, &msg) == 0, "the well-formed arrays are accepted");
    expect(validate(off, pos, HGX_JOIN_TYPE_SCAN, &msg) == 0, "... with the scan flag");
    expect(validate({0}, {}, 0, &msg) == 0, "a batch of 0 queries");
    expect(validate({0, 0, 0}, {}, 0, &msg) == 0, "queries without parts: part_pos is never read");
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
        {"part_off negative start", HGX_E_INVALID, "part_off[0]", {-1, 2, 2, 5}, pos, 0},
        {"part_off decreasing", HGX_E_INVALID, "decreases at join query 1", {0, 2, 1, 5}, pos, 0},
        {"part_off decreasing at the end", HGX_E_INVALID, "decreases at join query 2", {0, 2, 2, 1}, pos, 0},
        {"part_pos missing", HGX_E_INVALID, "null part_pos", off, {}, 0},
        {"a position below HGX_JOIN_SELF", HGX_E_INVALID, "join query 0 part 1", off, {0, -2, 3, 0, 1}, 0},
        {"... in the last part", HGX_E_INVALID, "join query 2 part 2", off, {0, -1, 3, 0, INT32_MIN}, 0},
        {"an unknown flag", HGX_E_INVALID, "unknown flag", off, pos, 2},
        {"a negative flag", HGX_E_INVALID, "unknown flag", off, pos, -1},
    };
    for (const Case& c : cases) {
        msg.clear();
        const int rc = validate(c.off, c.pos, c.flags, &msg);
        const bool ok = rc == c.code && msg.find(c.names) != std::string::npos;
        if (!ok) std::fprintf(stderr, "join_check: %s: status %d, message \"%s\"\n", c.what, rc, msg.c_str());
        expect(ok, c.what);
    }
    expect(validate({}, {}, 0, &msg) == HGX_E_INVALID, "a null part_off");
    expect(validate({0}, {}, 0, &msg, -1) == HGX_E_INVALID, "a negative query count");
    {   // more parts than a key's part field holds: refused before part_pos is read
        expect(validate({0, (int64_t)INT32_MAX - 1}, {}, 0, &msg) == HGX_E_UNSUPPORTED, "too many parts");
    }
    // the part field of a sort key holds the pad key's part, n_parts
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)3, (int64_t)4, (int64_t)255, (int64_t)256,
                      (int64_t)65535, (int64_t)65536, (int64_t)INT32_MAX - 2}) {
        const int32_t b = hgx::join_part_bits(n);
        expect(b >= 1 && b <= 31 && ((int64_t)1 << b) > n && (b == 1 || ((int64_t)1 << (b - 1)) <= n),
               "join_part_bits is the width of n_parts");
    }
    if (failures) return 1;
    std::printf("join_check: all checks passed\n");
    return 0;
}
