// sp_cpu.cc -- MEASUREMENT INFRASTRUCTURE for tools/sp_timing.py: a single-thread binary-heap Dijkstra over
// the snapshot arrays (the formulation of GraphClassics.dijkstra, core/src/java/org/hypergraphdb/algorithms/
// GraphClassics.java:126-209, with a heap for its TreeSet) and the generator's closed-form position rule
// (pyref.reachable) -- the CPU baseline the GPU shortest paths are timed against, and compared with bitwise.
#include <chrono>
#include <cstdint>
#include <limits>
#include <queue>
#include <utility>
#include <vector>

namespace {

struct Graph {
    int64_t A = 0, M = 0;
    const int64_t* tgt_off = nullptr;   // borrowed from the caller (kept alive by it)
    const int32_t* tgt_idx = nullptr;
    const int32_t* link_type = nullptr;
    std::vector<int64_t> inc_off;       // [A + 1]
    std::vector<int32_t> inc_row;       // one entry per distinct (target, link row), ascending rows
    std::vector<double> dist;           // [A] +inf between runs
    std::vector<int32_t> touched;
};

enum { kSym = 0, kAfterFirst = 1, kBeforeFirst = 2, kBeforeLast = 3, kAfterLast = 4 };

}  // namespace

extern "C" {

void* sp_cpu_build(int64_t A, int64_t M, const int64_t* tgt_off, const int32_t* tgt_idx, const int32_t* link_type) {
    Graph* g = new Graph();
    g->A = A;
    g->M = M;
    g->tgt_off = tgt_off;
    g->tgt_idx = tgt_idx;
    g->link_type = link_type;
    g->inc_off.assign((size_t)A + 1, 0);
    auto first_occurrence = [&](int64_t r, int64_t p) {
        for (int64_t q = tgt_off[r]; q < p; ++q)
            if (tgt_idx[q] == tgt_idx[p]) return false;
        return true;
    };
    for (int64_t r = 0; r < M; ++r)
        for (int64_t p = tgt_off[r]; p < tgt_off[r + 1]; ++p)
            if (first_occurrence(r, p)) ++g->inc_off[(size_t)tgt_idx[p] + 1];
    for (int64_t a = 0; a < A; ++a) g->inc_off[(size_t)a + 1] += g->inc_off[(size_t)a];
    g->inc_row.resize((size_t)g->inc_off[(size_t)A]);
    std::vector<int64_t> fill(g->inc_off.begin(), g->inc_off.end() - 1);
    for (int64_t r = 0; r < M; ++r)   // rows ascending: every incidence list comes out ascending
        for (int64_t p = tgt_off[r]; p < tgt_off[r + 1]; ++p)
            if (first_occurrence(r, p)) g->inc_row[(size_t)fill[(size_t)tgt_idx[p]]++] = (int32_t)r;
    g->dist.assign((size_t)A, std::numeric_limits<double>::infinity());
    return g;
}

void sp_cpu_free(void* h) { delete (Graph*)h; }

// Dijkstra for n pairs, one after the other on this thread.  goal < 0: the whole distance row, written to
// rows (A doubles per such pair, in pair order; may be null).  out_dist[i] = d(goal) (+inf: not connected;
// 0 for goal < 0).  Returns the seconds spent; *relaxed = edges examined.
double sp_cpu_run(void* h, int32_t mode, int32_t want_type, const double* w, const int32_t* starts, const int32_t* goals,
                  int32_t n, double* out_dist, double* rows, int64_t* relaxed) {
    Graph& g = *(Graph*)h;
    const double inf = std::numeric_limits<double>::infinity();
    int64_t n_relaxed = 0, row_i = 0;
    typedef std::pair<double, int32_t> Entry;   // (distance, atom): the TreeSet's (dm, handle) order
    const auto t0 = std::chrono::steady_clock::now();
    for (int32_t i = 0; i < n; ++i) {
        const int32_t start = starts[i], goal = goals[i];
        std::priority_queue<Entry, std::vector<Entry>, std::greater<Entry>> heap;
        g.dist[(size_t)start] = 0.0;
        g.touched.push_back(start);
        heap.push({0.0, start});
        double answer = goal < 0 ? 0.0 : inf;
        while (!heap.empty()) {
            const Entry top = heap.top();
            heap.pop();
            const int32_t a = top.second;
            if (top.first != g.dist[(size_t)a]) continue;   // a stale entry (lazy deletion)
            if (a == goal) {
                answer = top.first;
                break;
            }
            for (int64_t e = g.inc_off[(size_t)a]; e < g.inc_off[(size_t)a + 1]; ++e) {
                const int32_t r = g.inc_row[(size_t)e];
                if (want_type >= 0 && g.link_type[r] != want_type) continue;
                int64_t p = g.tgt_off[r], pe = g.tgt_off[r + 1];
                if (mode != kSym) {
                    int64_t fv = -1, lv = -1;
                    for (int64_t q = p; q < pe; ++q)
                        if (g.tgt_idx[q] == a) {
                            if (fv < 0) fv = q;
                            lv = q;
                        }
                    if (mode == kAfterFirst) p = fv + 1;
                    else if (mode == kBeforeFirst) pe = fv;
                    else if (mode == kBeforeLast) pe = lv;
                    else p = lv + 1;
                }
                const double nd = top.first + (w ? w[r] : 1.0);
                for (; p < pe; ++p) {
                    const int32_t t = g.tgt_idx[p];
                    if (t == a) continue;
                    ++n_relaxed;
                    if (nd < g.dist[(size_t)t]) {
                        if (g.dist[(size_t)t] == inf) g.touched.push_back(t);
                        g.dist[(size_t)t] = nd;
                        heap.push({nd, t});
                    }
                }
            }
        }
        out_dist[i] = answer;
        if (goal < 0 && rows) {
            double* row = rows + (row_i++) * g.A;
            for (int64_t k = 0; k < g.A; ++k) row[k] = inf;
            for (int32_t t : g.touched) row[t] = g.dist[(size_t)t];
        }
        for (int32_t t : g.touched) g.dist[(size_t)t] = inf;
        g.touched.clear();
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (relaxed) *relaxed = n_relaxed;
    return secs;
}

}  // extern "C"
