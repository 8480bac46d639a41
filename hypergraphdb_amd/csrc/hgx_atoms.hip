// hgx_atoms.hip -- the atom index behind hgx_pattern_batch_atoms (include/hgx_atoms.h): every atom of the
// snapshot, nodes and links, grouped by the atom-type column, in the record layout of the link index of
// hgx_scan.hip, so that the scan stage (hgx_scan_eval / hgx_scan_emit) reads either index.
//
// Replaces indexByType.find(T) over all atoms of a type (C/query/cond2qry/AndToQuery.java:120-294); the link index
// of hgx_scan.hip answers it for types without node instances only.
//
// GPU formulation, deterministic, plain vector stores, no atomic decides an order:
//   k_ai_init    -- a lane per atom: its id (the sort's values) and row_of[atom] = -1;
//   k_ai_scatter -- a lane per link row r: row_of[link_atom[r]] = r (link atoms are distinct: one writer a slot);
//   the sort     -- rocprim::radix_sort_pairs of (atom_type, atom): stable, so inside a type the atoms ascend;
//   the histogram-- rocprim::run_length_encode of the sorted keys: the distinct keys and their counts, copied to
//        the host, where the segment offsets are summed (as for the link index);
//   k_ai_fill    -- a lane per sorted atom: (atom, arity, first target offset) of its link row, or (atom, 0, 0,
//        kAtomNode) for a node.
// The filter on projected atoms lives in the join's keep kernel (hgx_join.hip); the entry point in hgx_query.hip.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>

#include "hgx_internal.h"

namespace hgx {

namespace {

__global__ void __launch_bounds__(256) k_ai_init(int64_t A, int32_t* __restrict__ atom, int32_t* __restrict__ row_of) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A; i += (int64_t)gridDim.x * blockDim.x) {
        atom[i] = (int32_t)i;
        row_of[i] = -1;
    }
}

__global__ void __launch_bounds__(256) k_ai_scatter(int64_t M, int64_t A, const int32_t* __restrict__ link_atom,
                                                    int32_t* __restrict__ row_of) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < M; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t la = link_atom[r];
        if (la >= 0 && la < A) row_of[la] = (int32_t)r;
    }
}

__global__ void __launch_bounds__(256) k_ai_fill(int64_t A, const int32_t* __restrict__ atom,
                                                 const int32_t* __restrict__ row_of,
                                                 const int64_t* __restrict__ tgt_off, int4* __restrict__ idx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t a = atom[i];
        const int32_t r = row_of[a];
        if (r < 0) {
            idx[i] = make_int4(a, 0, 0, kAtomNode);
        } else {
            const int64_t b = tgt_off[r], e = tgt_off[r + 1];
            idx[i] = make_int4(a, (int32_t)(e - b), (int32_t)(uint32_t)(b & 0xffffffffll), (int32_t)(b >> 32));
        }
    }
}

std::shared_ptr<AtomIndex> build_atom_index(hgx_graph* g) {
    auto ai = std::make_shared<AtomIndex>();
    const int64_t A = g->A, M = g->M;
    ai->seg.assign(1, 0);
    if (A == 0) return ai;
    hipStream_t s = g->stream;
    PoolScratch sc{g, {}};
    int32_t* atom = (int32_t*)sc.take(sizeof(int32_t) * A);
    int32_t* atom2 = (int32_t*)sc.take(sizeof(int32_t) * A);
    int32_t* row_of = (int32_t*)sc.take(sizeof(int32_t) * A);
    int32_t* key2 = (int32_t*)sc.take(sizeof(int32_t) * A);
    int32_t* uniq = (int32_t*)sc.take(sizeof(int32_t) * A);
    unsigned int* cnt = (unsigned int*)sc.take(sizeof(unsigned int) * A);
    int64_t* nruns = (int64_t*)sc.take(sizeof(int64_t));
    k_ai_init<<<grid_for(A, 256, 4096), 256, 0, s>>>(A, atom, row_of);
    HGX_CHECK_LAUNCH();
    if (M > 0) {
        k_ai_scatter<<<grid_for(M, 256, 4096), 256, 0, s>>>(M, A, g->link_atom, row_of);
        HGX_CHECK_LAUNCH();
    }
    // a radix sort is stable: inside a type the atoms stay ascending (the keys are not negative)
    size_t tb = 0;
    HGX_HIP(rocprim::radix_sort_pairs(nullptr, tb, g->atom_type, key2, atom, atom2, (size_t)A, 0u, 32u, s));
    void* tmp = sc.take(tb);
    HGX_HIP(rocprim::radix_sort_pairs(tmp, tb, g->atom_type, key2, atom, atom2, (size_t)A, 0u, 32u, s));
    size_t rb = 0;
    HGX_HIP(rocprim::run_length_encode(nullptr, rb, key2, (unsigned int)A, uniq, cnt, nruns, s));
    void* rtmp = sc.take(rb);
    HGX_HIP(rocprim::run_length_encode(rtmp, rb, key2, (unsigned int)A, uniq, cnt, nruns, s));
    HGX_HIP(hipMalloc(&ai->idx, sizeof(int4) * (size_t)A));   // (freed with the object on every error path)
    k_ai_fill<<<grid_for(A, 256, 4096), 256, 0, s>>>(A, atom2, row_of, g->tgt_off, ai->idx);
    HGX_CHECK_LAUNCH();
    int64_t nr = 0;
    HGX_HIP(hipMemcpyAsync(&nr, nruns, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HGX_HIP(hipStreamSynchronize(s));
    if (nr < 1 || nr > A) fail(HGX_E_DEVICE, "atom index: bad histogram");
    std::vector<unsigned int> hc((size_t)nr);
    ai->key.resize((size_t)nr);
    HGX_HIP(hipMemcpyAsync(ai->key.data(), uniq, sizeof(int32_t) * (size_t)nr, hipMemcpyDeviceToHost, s));
    HGX_HIP(hipMemcpyAsync(hc.data(), cnt, sizeof(unsigned int) * (size_t)nr, hipMemcpyDeviceToHost, s));
    HGX_HIP(hipStreamSynchronize(s));
    ai->seg.resize((size_t)nr + 1);
    for (int64_t i = 0; i < nr; ++i) ai->seg[i + 1] = ai->seg[i] + (int64_t)hc[i];
    if (ai->seg[nr] != A) fail(HGX_E_DEVICE, "atom index: the histogram does not cover the atoms");
    return ai;
}

std::string no_types(const char* who) {
    return std::string(who) + ": the snapshot has no atom types (hgx_graph_set_atom_types)";
}

}  // namespace

std::shared_ptr<AtomIndex> ensure_atom_index(hgx_graph* g, const char* who) {
    if (g->base) {   // an execution context: the snapshot builds the index once; the context holds a reference
        hgx_graph* b = g->base;
        std::lock_guard<std::mutex> lk(b->mu);   // lock order: context, then its snapshot (never the reverse)
        HGX_HIP(hipSetDevice(b->device));
        g->atom_index = ensure_atom_index(b, who);
        return g->atom_index;
    }
    if (!g->atom_type) fail(HGX_E_UNSUPPORTED, no_types(who));
    if (!g->atom_index) g->atom_index = build_atom_index(g);
    return g->atom_index;
}

void atoms_require_types(hgx_graph* g, const char* who) {
    hgx_graph* root = g->base ? g->base : g;
    std::lock_guard<std::mutex> lk(root->mu);
    if (!root->atom_type) fail(HGX_E_UNSUPPORTED, no_types(who));
}

int64_t atoms_keep_validate(const hgx_graph* g, int32_t n_queries, hgx_atom_predicate* const* keep) {
    const hgx_graph* root = g->base ? g->base : g;
    int64_t n = 0;
    for (int32_t j = 0; j < n_queries; ++j) {
        if (!keep[j]) continue;
        if (keep[j]->root != root)
            fail(HGX_E_INVALID, "hgx_pattern_batch_atoms: join query " + std::to_string(j) +
                                    ": the atom predicate was made on another graph");
        ++n;
    }
    return n;
}

}  // namespace hgx

using namespace hgx;

extern "C" int hgx_graph_type_atoms(hgx_graph* g, const int32_t* types, int64_t n, int64_t* out_counts) {
    HGX_API_BEGIN
    if (!g || n < 0 || (n > 0 && (!types || !out_counts))) fail(HGX_E_INVALID, "hgx_graph_type_atoms: bad argument");
    if (g->shard) fail(HGX_E_UNSUPPORTED, "hgx_graph_type_atoms: not available on a partition shard");
    std::lock_guard<std::mutex> lk(g->mu);
    HGX_HIP(hipSetDevice(g->device));
    const std::shared_ptr<AtomIndex> ai = ensure_atom_index(g, "hgx_graph_type_atoms");
    for (int64_t i = 0; i < n; ++i) {
        const auto it = std::lower_bound(ai->key.begin(), ai->key.end(), types[i]);
        const size_t k = (size_t)(it - ai->key.begin());
        out_counts[i] = (it != ai->key.end() && *it == types[i]) ? ai->seg[k + 1] - ai->seg[k] : 0;
    }
    HGX_API_END
}
