/* CPU model of the batched BFS level engine's work: the config-2 / config-4
 * generator of hgx_gen.c, S-bit rows, incidence lists deduplicated and ascending, hubs at degree > 512,
 * the cover test acc | vis == FULL.  Per level it prints the frontier, the active links and frontier pins
 * (what the link gather reads), and per exit step E = 1/2/4/8/16 the lf rows a pull of gather + pull
 * reads, the frontier rows a direct pull reads (own row included; entries) and the links whose lf row
 * any pull reads -- light atoms and hubs apart.  Item 13's hint columns follow: how concentrated the
 * neighbour hints are, and per level the listed atoms that vis | lvl[hint] covers (with one hint, with a
 * second), and the entry walk left to the atoms they do not cover, per exit step.
 * Item 14's hub-mask columns: per level and T = 8/16/32/64, |C|, the fr atoms and their degree sum, the links
 * with an fr atom, the hub entries walked until a chunk's block-wide test passes and the lr-set share after it.
 *   gcc -O3 -fopenmp -o bfs_level_model tools/bfs_level_model.c hypergraphdb_amd/csrc/hgx_gen.c -lm
 *   ./bfs_level_model [scale=0.01] [sources=1024] [depth=4] [nodes=10e6*scale] [links=40e6*scale]   */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int64_t hgx_gen_hypergraph_offsets(int64_t M, int32_t lo, int32_t hi, uint64_t seed, int64_t *tgt_off);
int hgx_gen_hypergraph_fill(int64_t N, int64_t M, int32_t lo, int32_t hi, double gamma, int32_t n_types,
                            uint64_t seed, const int64_t *tgt_off, int32_t *tgt_idx, int32_t *link_type);
int hgx_gen_sources(int64_t n, int64_t P, const int32_t *tgt_idx, int64_t k, uint64_t seed, int32_t *out);

enum { NE = 5, HEAVY = 512 };
static const int ES[NE] = {1, 2, 4, 8, 16};
enum { NT = 4 };
static const int TS[NT] = {8, 16, 32, 64};
typedef uint64_t u64;

static int cmp_desc(const void *a, const void *b) {
    const int64_t x = *(const int64_t *)a, y = *(const int64_t *)b;
    return x < y ? 1 : x > y ? -1 : 0;
}

int main(int argc, char **argv) {
    const double scale = argc > 1 ? atof(argv[1]) : 0.01;
    const int S = argc > 2 ? atoi(argv[2]) : 1024, depth = argc > 3 ? atoi(argv[3]) : 4, W = (S + 63) / 64;
    const int64_t N = argc > 4 ? atoll(argv[4]) : (int64_t)(10e6 * scale), M = argc > 5 ? atoll(argv[5]) : (int64_t)(40e6 * scale);
    int64_t *off = malloc(sizeof(int64_t) * (M + 1));
    const int64_t P = hgx_gen_hypergraph_offsets(M, 2, 8, 42, off);
    int32_t *tg = malloc(sizeof(int32_t) * P), *lt = malloc(sizeof(int32_t) * M), *seeds = malloc(sizeof(int32_t) * S);
    if (hgx_gen_hypergraph_fill(N, M, 2, 8, 2.1, 1, 42, off, tg, lt) || hgx_gen_sources(N, P, tg, S, 7, seeds)) return 1;
    /* incidence: links ascending, a link listed once per atom */
    int64_t *io = calloc(N + 1, sizeof(int64_t));
    int32_t *last = malloc(sizeof(int32_t) * N), *inc = NULL;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass) {
            for (int64_t v = 0; v < N; ++v) io[v + 1] += io[v];
            inc = malloc(sizeof(int32_t) * (io[N] + 1));
        }
        memset(last, 0xff, sizeof(int32_t) * N);
        for (int64_t L = 0; L < M; ++L)
            for (int64_t p = off[L]; p < off[L + 1]; ++p) {
                const int32_t v = tg[p];
                if (last[v] == (int32_t)L) continue;
                last[v] = (int32_t)L;
                if (pass) inc[io[v]++] = (int32_t)L; else ++io[v + 1];
            }
        if (pass) {
            for (int64_t v = N; v > 0; --v) io[v] = io[v - 1];
            io[0] = 0;
        }
    }
    /* neighbour hints (item 13): per atom the co-targets u != t of largest and second largest (degree, id)
     * over every link of inc(t), -1 = none -- a property of the snapshot */
    int32_t *hint1 = malloc(sizeof(int32_t) * N), *hint2 = malloc(sizeof(int32_t) * N);
    int64_t n_inc = 0;
#pragma omp parallel for schedule(dynamic, 256) reduction(+ : n_inc)
    for (int64_t t = 0; t < N; ++t) {
        u64 k1 = 0, k2 = 0;
        for (int64_t i = io[t]; i < io[t + 1]; ++i)
            for (int64_t p = off[inc[i]]; p < off[inc[i] + 1]; ++p) {
                const int32_t u = tg[p];
                if (u == t) continue;
                const u64 key = ((u64)(io[u + 1] - io[u]) << 32) | (uint32_t)u;
                if (key > k1) { k2 = k1; k1 = key; }
                else if (key > k2 && key != k1) k2 = key;
            }
        hint1[t] = k1 ? (int32_t)(uint32_t)k1 : -1;
        hint2[t] = k2 ? (int32_t)(uint32_t)k2 : -1;
        n_inc += io[t + 1] > io[t];
    }
    {   /* how concentrated the hints are: distinct hint atoms, and the share served by the top ones */
        int64_t *use = calloc(N, sizeof(int64_t)), distinct = 0, top = 0;
        for (int64_t t = 0; t < N; ++t) if (hint1[t] >= 0) ++use[hint1[t]];
        qsort(use, N, sizeof(int64_t), cmp_desc);
        while (distinct < N && use[distinct]) ++distinct;
        printf("hints: %lld atoms with incidence, %lld distinct hint atoms; served by the top", (long long)n_inc, (long long)distinct);
        const int64_t marks[3] = {64, 1024, 32768};
        for (int64_t r = 0, m = 0; r < distinct && m < 3; ++r) {
            top += use[r];
            if (r + 1 == marks[m] || r + 1 == distinct) {
                printf(" %lld: %.1f%%", (long long)(r + 1), 100.0 * top / (n_inc ? n_inc : 1));
                ++m;
            }
        }
        printf("\n");
        free(use);
    }
    u64 FULL[16] = {0};
    for (int s = 0; s < S; ++s) FULL[s >> 6] |= 1ull << (s & 63);
    u64 *vis = calloc((size_t)N * W, 8), *lvl = calloc((size_t)N * W, 8), *nxt = calloc((size_t)N * W, 8);
    uint8_t *F = calloc(N, 1), *Fn = calloc(N, 1), *used = malloc((size_t)M * NE);
    for (int s = 0; s < S; ++s) {
        lvl[(size_t)seeds[s] * W + (s >> 6)] |= 1ull << (s & 63);
        vis[(size_t)seeds[s] * W + (s >> 6)] |= 1ull << (s & 63);
        F[seeds[s]] = 1;
    }
    /* the snapshot's top list (item 14): the 64 atoms of largest (degree, id), descending */
    int32_t top[64];
    int ntop = 0;
    uint8_t *frm = malloc(N), *lrm = malloc(M);
    {
        int64_t *key = malloc(sizeof(int64_t) * N);
        for (int64_t v = 0; v < N; ++v) key[v] = ((io[v + 1] - io[v]) << 32) | v;
        qsort(key, N, sizeof(int64_t), cmp_desc);
        for (; ntop < 64 && ntop < N; ++ntop) top[ntop] = (int32_t)(key[ntop] & 0xffffffff);
        free(key);
    }
    printf("N %lld M %lld P %lld I %lld S %d\n", (long long)N, (long long)M, (long long)P, (long long)io[N], S);
    for (int d = 0; d < depth; ++d) {
        int64_t nf = 0, alinks = 0, fpins = 0, nnew = 0, cand[2] = {0, 0}, k1[2] = {0, 0}, cover[2] = {0, 0};
        int64_t lf[2][NE] = {{0}}, rows[2][NE] = {{0}}, ent[2][NE] = {{0}};
        /* hints: listed atoms covered by vis | lvl[hint1], by that | lvl[hint2]; the walk left to the rest */
        int64_t hcov1[2] = {0, 0}, hcov2[2] = {0, 0}, r1ent[NE] = {0}, r1rows[NE] = {0}, r2ent[NE] = {0}, r2rows[NE] = {0};
        for (int64_t v = 0; v < N; ++v) nf += F[v];
#pragma omp parallel for reduction(+ : alinks, fpins) schedule(static, 4096)
        for (int64_t L = 0; L < M; ++L) {
            int c = 0;
            for (int64_t p = off[L]; p < off[L + 1]; ++p) c += F[tg[p]];
            alinks += c > 0;
            fpins += c;
        }
        /* hub mask (item 14), per T: C = OR of the level rows of the first T top-list atoms on the frontier; the
         * fr atoms (frontier atoms with a bit outside C) and their degree sum; the links with an fr atom; per hub
         * chunk of 4096 entries, one accumulator and the test acc | vis ⊇ C after every 256 entries: the entries
         * walked until it passes, the entries after it and how many of those have an fr link */
        for (int ti = 0; ti < NT; ++ti) {
            u64 C[16] = {0};
            int listed = 0, pc = 0;
            for (int k = 0; k < TS[ti] && k < ntop; ++k)
                if (F[top[k]]) { ++listed; for (int w = 0; w < W; ++w) C[w] |= lvl[(size_t)top[k] * W + w]; }
            for (int w = 0; w < W; ++w) pc += __builtin_popcountll(C[w]);
            int64_t nfr = 0, frdeg = 0, frlinks = 0, before = 0, after = 0, after_lr = 0, hub_entries = 0;
            memset(frm, 0, N);
#pragma omp parallel for reduction(+ : nfr, frdeg) schedule(static, 4096)
            for (int64_t v = 0; v < N; ++v) {
                if (!F[v]) continue;
                u64 o = 0;
                for (int w = 0; w < W; ++w) o |= lvl[(size_t)v * W + w] & ~C[w];
                if (o) { frm[v] = 1; ++nfr; frdeg += io[v + 1] - io[v]; }
            }
#pragma omp parallel for reduction(+ : frlinks) schedule(static, 4096)
            for (int64_t L = 0; L < M; ++L) {
                int c = 0;
                for (int64_t p = off[L]; p < off[L + 1]; ++p) c |= frm[tg[p]];
                lrm[L] = (uint8_t)c;
                frlinks += c;
            }
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : before, after, after_lr, hub_entries)
            for (int64_t t = 0; t < N; ++t) {
                const int64_t b = io[t], e = io[t + 1];
                if (e - b <= HEAVY) continue;
                const u64 *vt = vis + (size_t)t * W;
                int full = 1;
                for (int w = 0; w < W; ++w) full &= vt[w] == FULL[w];
                if (full) continue;
                hub_entries += e - b;
                for (int64_t cb = b; cb < e; cb += 4096) {
                    const int64_t ce = cb + 4096 < e ? cb + 4096 : e;
                    u64 acc[16] = {0};
                    int64_t i = cb;
                    int pass = 0;
                    for (; i < ce && !pass;) {
                        const int64_t se = i + 256 < ce ? i + 256 : ce;
                        for (; i < se; ++i)
                            for (int64_t p = off[inc[i]]; p < off[inc[i] + 1]; ++p)
                                if (F[tg[p]]) for (int w = 0; w < W; ++w) acc[w] |= lvl[(size_t)tg[p] * W + w];
                        pass = listed > 0;
                        for (int w = 0; w < W; ++w) pass &= ((acc[w] | vt[w] | ~C[w]) & FULL[w]) == FULL[w];
                    }
                    before += i - cb;
                    for (; i < ce; ++i) { ++after; after_lr += lrm[inc[i]]; }
                }
            }
            printf("  hub mask T=%-2d: listed on the frontier %d |C| %d; fr atoms %lld degree sum %lld; links with an fr atom %lld; "
                   "hub entries %lld: before the switch %lld, after %lld of which lr-set %lld (%.1f%%)\n", TS[ti], listed, pc,
                   (long long)nfr, (long long)frdeg, (long long)frlinks, (long long)hub_entries, (long long)before,
                   (long long)after, (long long)after_lr, after ? 100.0 * after_lr / after : 0.0);
        }
        memset(used, 0, (size_t)M * NE);
        memset(nxt, 0, (size_t)N * W * 8);
#pragma omp parallel for schedule(dynamic, 256) reduction(+ : nnew, cand[:2], k1[:2], cover[:2], lf[:2][:NE], rows[:2][:NE], ent[:2][:NE], hcov1[:2], hcov2[:2], r1ent[:NE], r1rows[:NE], r2ent[:NE], r2rows[:NE])
        for (int64_t t = 0; t < N; ++t) {
            const int64_t b = io[t], e = io[t + 1], deg = e - b;
            u64 *vt = vis + (size_t)t * W, acc[16] = {0};
            int full = 1;
            for (int w = 0; w < W; ++w) full &= vt[w] == FULL[w];
            Fn[t] = 0;
            if (deg == 0 || full) continue;
            const int h = deg > HEAVY;
            int64_t kc = deg;   /* entries until acc | vis covers (deg: never) */
            int covered = 0;
            for (int64_t i = 0; i < deg && !covered; ++i) {
                const int32_t L = inc[b + i];
                for (int64_t p = off[L]; p < off[L + 1]; ++p)
                    if (F[tg[p]]) for (int w = 0; w < W; ++w) acc[w] |= lvl[(size_t)tg[p] * W + w];
                covered = 1;
                for (int w = 0; w < W; ++w) covered &= (acc[w] | vt[w]) == FULL[w];
                if (covered) kc = i + 1;
            }
            ++cand[h];
            cover[h] += covered;
            int c1 = 0, c2 = 0;
            {
                const int32_t h1 = hint1[t], h2 = hint2[t];
                u64 a[16];
                for (int w = 0; w < W; ++w) a[w] = vt[w];
                if (h1 >= 0 && F[h1]) {
                    c1 = 1;
                    for (int w = 0; w < W; ++w) { a[w] |= lvl[(size_t)h1 * W + w]; c1 &= a[w] == FULL[w]; }
                }
                c2 = c1;
                if (!c1 && h2 >= 0 && F[h2]) {
                    c2 = 1;
                    for (int w = 0; w < W; ++w) { a[w] |= lvl[(size_t)h2 * W + w]; c2 &= a[w] == FULL[w]; }
                }
                hcov1[h] += c1;
                hcov2[h] += c2;
            }
            k1[h] += kc;
            for (int64_t i = 0; i < deg && i < (kc + 15) / 16 * 16; ++i) {
                const int32_t L = inc[b + i];
                int c = 0;
                for (int64_t p = off[L]; p < off[L + 1]; ++p) c += F[tg[p]];
                for (int k = 0; k < NE; ++k) {
                    const int64_t stop = (kc + ES[k] - 1) / ES[k] * ES[k];
                    if (i >= stop) continue;
                    ++ent[h][k];
                    rows[h][k] += c;
                    if (!c1) { ++r1ent[k]; r1rows[k] += c; }
                    if (!c2) { ++r2ent[k]; r2rows[k] += c; }
                    if (c) { ++lf[h][k]; used[(size_t)L * NE + k] = 1; }
                }
            }
            int any = 0;
            for (int w = 0; w < W; ++w) {
                const u64 nw = acc[w] & ~vt[w];
                nxt[(size_t)t * W + w] = nw;
                any |= nw != 0;
            }
            if (any) { Fn[t] = 1; ++nnew; for (int w = 0; w < W; ++w) vt[w] |= acc[w]; }
        }
        printf("level %d: frontier %lld atoms, active links %lld (%.1f%%), frontier pins %lld, new atoms %lld\n", d,
               (long long)nf, (long long)alinks, 100.0 * alinks / M, (long long)fpins, (long long)nnew);
        for (int h = 0; h < 2; ++h) {
            printf("  %s: %lld not full, %lld cover, entries to cover (sum) %lld\n", h ? "hubs " : "light", (long long)cand[h],
                   (long long)cover[h], (long long)k1[h]);
            for (int k = 0; k < NE; ++k)
                printf("    E=%-2d entries %lld  lf rows %lld  direct rows %lld\n", ES[k], (long long)ent[h][k],
                       (long long)lf[h][k], (long long)rows[h][k]);
        }
        printf("  hints: covered by vis | lvl[hint] light %lld hubs %lld; with a second hint light %lld hubs %lld\n",
               (long long)hcov1[0], (long long)hcov1[1], (long long)hcov2[0], (long long)hcov2[1]);
        for (int k = 0; k < NE; ++k)
            printf("    E=%-2d walk left after one hint: entries %lld direct rows %lld; after two: entries %lld direct rows %lld\n",
                   ES[k], (long long)r1ent[k], (long long)r1rows[k], (long long)r2ent[k], (long long)r2rows[k]);
        for (int k = 0; k < NE; ++k) {
            int64_t u = 0;
            for (int64_t L = 0; L < M; ++L) u += used[(size_t)L * NE + k];
            printf("  E=%-2d links whose row a pull reads %lld (%.1f%% of the active links)\n", ES[k], (long long)u,
                   alinks ? 100.0 * u / alinks : 0.0);
        }
        u64 *x = lvl; lvl = nxt; nxt = x;
        uint8_t *y = F; F = Fn; Fn = y;
        if (!nnew) break;
    }
    return 0;
}
