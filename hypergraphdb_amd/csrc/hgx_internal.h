// hgx_internal.h -- shared definitions of the MI355X engine (libhgx.so).
//
// Device layout of a snapshot:
//   link_atom [M]   int32   atom id of link row r (ascending)
//   tgt_off   [M+1] int64   target row offsets
//   tgt_idx   [P]   int32   target atom ids, layout order t0..tk-1
//   link_type [M]   int32   type key of link row r
//   inc_off   [A+1] int64   incidence row offsets
//   inc_row   [I]   int32   incident LINK ROWS, ascending (row order == atom rank order)
//   inc_type  [I]   int32   type key of inc_row[i] (denormalised for the pattern filter)
// plus the heavy-atom chunk table used to balance power-law incidence rows.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hgx_atoms.h"
#include "../../include/hgx_dnf.h"
#include "../../include/hgx_hops.h"
#include "../../include/hgx_join.h"
#include "../../include/hgx_linkpred.h"
#include "../../include/hgx_not.h"
#include "../../include/hgx_paths.h"
#include "../../include/hgx_scan.h"
#include "../../include/hgx_sets.h"
#include "../../include/hgx_sibling.h"

namespace hgx {

typedef unsigned long long u64;

// Engine knobs.  The product library reads no tuning setting from the environment (a library loaded into
// a JVM must not change behaviour with whichever call read the environment first, and getenv racing a
// setenv is undefined in a multi-threaded host): tunables that callers and tests set go through
// hgx_set_option (per graph).  The measured-negative A/B variants of DESIGN.md are reachable only in A/B
// builds (tools/build_variant.sh compiles with -DHGX_AB_KNOBS), where ab_env reads them; tracing
// (trace_env: HGX_BFS_TRACE, HGX_SEQ_TRACE, HGX_CO_TRACE, HGX_LS_PROF, HGX_QUERY_PROFILE) stays
// environment-driven and only adds output.
inline const char* ab_env(const char* name) {
#ifdef HGX_AB_KNOBS
    return std::getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}
inline bool trace_env(const char* name) { return std::getenv(name) != nullptr; }
inline int ab_int(const char* name, int dflt) {
    const char* e = ab_env(name);
    return e ? std::atoi(e) : dflt;
}

struct Error {
    int code;
    std::string msg;
};

[[noreturn]] void fail(int code, const std::string& msg);
void set_last_error(const std::string& msg);

#define HGX_HIP(x)                                                                              \
    do {                                                                                        \
        hipError_t e_ = (x);                                                                    \
        if (e_ != hipSuccess)                                                                   \
            ::hgx::fail(HGX_E_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_));          \
    } while (0)

#define HGX_CHECK_LAUNCH() HGX_HIP(hipGetLastError())

#define HGX_API_BEGIN try {
// As HGX_API_END without the final `return HGX_OK` (a body that falls through to more code).
#define HGX_API_END_NORETURN                                                                    \
    }                                                                                           \
    catch (const ::hgx::Error& e) {                                                             \
        ::hgx::set_last_error(e.msg);                                                           \
        return e.code;                                                                          \
    }                                                                                           \
    catch (const std::bad_alloc&) {                                                             \
        ::hgx::set_last_error("host allocation failed");                                        \
        return HGX_E_NOMEM;                                                                     \
    }                                                                                           \
    catch (const std::exception& e) {                                                           \
        ::hgx::set_last_error(e.what());                                                        \
        return HGX_E_DEVICE;                                                                    \
    }                                                                                           \
    catch (...) {                                                                               \
        ::hgx::set_last_error("unknown error");                                                 \
        return HGX_E_DEVICE;                                                                    \
    }

#define HGX_API_END                                                                             \
    }                                                                                           \
    catch (const ::hgx::Error& e) {                                                             \
        ::hgx::set_last_error(e.msg);                                                           \
        return e.code;                                                                          \
    }                                                                                           \
    catch (const std::bad_alloc&) {                                                             \
        ::hgx::set_last_error("host allocation failed");                                        \
        return HGX_E_NOMEM;                                                                     \
    }                                                                                           \
    catch (const std::exception& e) {                                                           \
        ::hgx::set_last_error(e.what());                                                        \
        return HGX_E_DEVICE;                                                                    \
    }                                                                                           \
    catch (...) {                                                                               \
        ::hgx::set_last_error("unknown error");                                                 \
        return HGX_E_DEVICE;                                                                    \
    }                                                                                           \
    return HGX_OK;

// Incidence rows longer than this are split into chunks processed by whole workgroups.
constexpr int64_t kHeavyDegree = 512;
constexpr int64_t kChunkEntries = 4096;

struct HeavyChunk {
    int64_t beg, end;   // incidence entry range
    int32_t atom;       // atom id
    int32_t slot;       // heavy-atom slot (accumulator row)
};

struct PoolBuf {
    void* p;
    size_t n;
};

// A yield list (yield_list below): the links of each atom's incidence entries that pass one link type
// and can yield in one generator mode, in entry order.
struct YieldList {
    int32_t mode, type;
    int64_t* off;   // [A + 1]
    int32_t* row;   // [n] link ids
    int64_t n;
};
constexpr size_t kMaxYieldLists = 8;

// A yield adjacency (yield_adj below): per atom, the generator's output itself -- every (target, link
// atom) pair its incidence entries yield in one mode for one link type and minimum arity, in stream
// order (entry order, then yield rank).  off == nullptr: refused (more than kYieldAdjBudget bytes).
struct YieldAdj {
    int32_t mode, type, min_arity, rev;
    int64_t* off;   // [A + 1]
    int32_t* tgt;   // [n]
    int32_t* lnk;   // [n] link atom ids
    int64_t n;
};
constexpr int64_t kYieldAdjBudget = (int64_t)4 << 30;

// Vertex-cut partition of a snapshot over n_parts devices (hgx_part.hip):
// every link row lives on one part; an atom is present (local) on every part holding one of its
// links and owned by one of them.  Local ids are assigned in global id order, so every ascending
// local list is an ascending global list.
struct ShardInfo {
    int32_t n_parts = 1, part = 0;
    int64_t A_global = 0, n_owned = 0;
    std::vector<int32_t> l2g_host;       // [A_local] global id of local atom (ascending)
    std::vector<uint64_t> present_host;  // [A_global/64 + 1] atoms present on some part
    std::vector<uint64_t> own_bm_host;   // [A_local/64 + 2] bit set <=> local atom is owned here
    std::vector<int64_t> ghost_count;    // [n_parts] my ghosts owned by part q = reduce records to q (max)
    std::vector<int64_t> bc_count;       // [n_parts] my owned atoms held by part q = broadcast records to q (max)
    bool serial = false;                 // in-process rehearsal: parts run their kernels one at a time
    // device copies
    uint64_t* own_bm = nullptr;          // [A_local/64 + 2]
    int32_t* xo_part = nullptr;          // [A_local] ghost: owner part (-1 owned)
    int32_t* xo_lid = nullptr;           // [A_local] ghost: its local id on the owner
    int64_t* bc_off = nullptr;           // [A_local + 1] owned atom: its other holders ...
    int32_t* bc_part = nullptr;          //   ... their parts
    int32_t* bc_lid = nullptr;           //   ... and its local id there
    // Static exchange slots (dense levels): the j-th of my ghosts owned by q (ascending ids) sends to
    // slot j of q's receive segment from me, and q's j-th owned atom held by me (ascending ids: the
    // same atom) answers in slot j of my receive segment from q.
    int32_t* bc_slot = nullptr;          // [bc entries] its slot in the (me -> holder) segment
    int32_t* bc_atom = nullptr;          // [bc entries] the owned atom of the entry (flat broadcast pack)
    int32_t xmode = 1;                   // HGX_OPT_PART_EXCHANGE: 0 / 1 compressed records (static slots removed in round 5)
    // the global -> local id of an atom present here, or -1 (binary search of l2g_host)
    int32_t local_of(int64_t v) const {
        auto it = std::lower_bound(l2g_host.begin(), l2g_host.end(), (int32_t)v);
        return (it != l2g_host.end() && *it == v) ? (int32_t)(it - l2g_host.begin()) : -1;
    }
    bool owns_local(int64_t l) const { return (own_bm_host[l >> 6] >> (l & 63)) & 1ull; }
    bool present(int64_t v) const { return (present_host[v >> 6] >> (v & 63)) & 1ull; }
};

// Transport of the per-level frontier exchange: RCCL between processes (one GPU each), an
// in-process group of shard threads, or host-staged callbacks.  Every call is collective.
struct Transport {
    int32_t world = 1, rank = 0;
    virtual ~Transport() {}
    // out[r * n + i] = in[i] of rank r (host buffers)
    virtual void allgather_i64(const int64_t* in, int64_t n, int64_t* out, hipStream_t s) = 0;
    // The same for a DEVICE input written by work ordered on s: out (host) = every rank's n values;
    // pin = pinned host scratch of n * world int64.  Returns the host round trips it took.  The
    // default reads the values back and runs the host all-gather (two); RCCL gathers on the device
    // and reads the gathered block back once (hgx_part.hip).
    virtual int allgather_dev(const int64_t* din, int64_t n, int64_t* out, hipStream_t s, int64_t* pin);
    // rank p receives send_bytes[p] bytes from send + send_off[p]; this rank receives recv_bytes[p]
    // bytes from rank p at recv + recv_off[p] (device buffers, ordered on stream s)
    virtual void alltoallv(const void* send, const int64_t* send_off, const int64_t* send_bytes, void* recv,
                           const int64_t* recv_off, const int64_t* recv_bytes, hipStream_t s) = 0;
    // brackets of a part's device work between two exchanges (the in-process rehearsal runs the
    // parts' kernels one part at a time so their device times are clean)
    virtual void compute_begin(hipStream_t) {}
    virtual void compute_end(hipStream_t) {}
    virtual void compute_release(hipStream_t) {}   // end of the work or an error path: give the gate back
    virtual const char* kind() const = 0;
};
// A part's device work between compute_begin and compute_release (tr may be null: one part); the gate is given
// back on an error path too.
struct ComputeGate {
    Transport* tr;
    hipStream_t s;
    ComputeGate(Transport* t, hipStream_t st) : tr(t), s(st) {
        if (tr) tr->compute_begin(s);
    }
    ~ComputeGate() {
        if (tr) tr->compute_release(s);
    }
};

// Cross-thread coalescing of pattern batches (hgx_pattern_batch_packed, HGX_OPT_QUERY_COALESCE):
// a caller that finds the graph's device busy queues its batch; whoever runs next takes every queued
// batch (FIFO, up to a query cap) and runs them as ONE device batch, then splits the result.  The
// reference's usage is many threads each executing small compiled queries
// (TC/query/QueryCompilation.java:76-122); one device batch per caller would serialise them on the
// per-graph mutex at the full fixed cost of a batch each.
struct PackedReq {
    int32_t n = 0;
    const int32_t* type = nullptr;
    const int64_t* inc_off = nullptr;
    const int32_t* inc = nullptr;
    const int32_t* has_ordered = nullptr;
    const int64_t* pat_off = nullptr;
    const int32_t* pat = nullptr;
    hgx_query_result* r = nullptr;   // set when done and rc == HGX_OK
    int rc = HGX_OK;
    std::string err;
    bool done = false;
};
struct QueryCombiner {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<PackedReq*> pending;
    bool busy = false;
    int64_t batches = 0, requests = 0;   // device batches run / caller batches served (statistics)
};

}  // namespace hgx

namespace hgx {
// The atom index (include/hgx_atoms.h, hgx_atoms.hip): one 16-byte record per atom in the layout of the link
// index -- (atom, arity, first target offset low / high word); a node: arity 0 and the high word kAtomNode -- the
// atoms stably sorted by atom_type, so a type is one segment whose atoms ascend.  key / seg: the sorted distinct
// type keys and their segment offsets, on the host.  Shared: a context holds a reference on its snapshot's index,
// so a replaced atom-type column never frees an index a context's batch still reads.
constexpr int32_t kAtomNode = -1;
struct AtomIndex {
    int4* idx = nullptr;          // [A]
    std::vector<int32_t> key;     // [n distinct types] ascending
    std::vector<int64_t> seg;     // [n distinct types + 1]
    ~AtomIndex() {
        if (idx) (void)hipFree(idx);
    }
};
}  // namespace hgx

struct hgx_comm {
    hgx::Transport* t = nullptr;
};

struct hgx_graph {
    // Execution context (hgx_graph_context): the snapshot's arrays are borrowed from base (which this
    // context holds a reference on); the stream, lock, scratch pool, accumulator, counters and host
    // staging are its own, so traversals on two contexts of one snapshot run side by side.
    hgx_graph* base = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;      // readout counting next to the traversal (made on first use)
    hipStream_t stream3 = nullptr;      // the order-exact level engine's second copy stream (made on first use)
    hipEvent_t ev_count = nullptr;      //   and its ordering event
    std::mutex mu;
    std::atomic<int> refs{1};
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;   // timing events reused across calls (taken under mu)
    int32_t bfs_flags = 0x3BE;      // HGX_OPT_BFS_FLAGS (see hgx.h)
    int64_t seq_budget_bytes = (int64_t)48 << 30;   // HGX_OPT_SEQ_BUDGET: order-exact traversal working set
    int64_t max_arity = -1, max_deg = -1;           // lazily computed (order-exact stream keys)
    int32_t seq_engine = 0;                         // HGX_OPT_SEQ_ENGINE: 0 workgroup per seed (+ level engine), 1 key-array
                                                    //   level engine only, 2 level engine (hgx_ls_*) only
    unsigned long long* seq_flag = nullptr;         // mapped coherent words: level sizes of the level engine
    hipEvent_t ls_ev[16] = {};                      //   its rank parts' events (2 level parities x 8 parts)
    hipEvent_t ls_cev[2] = {};                      //   a level's pair copies enqueued (by level parity)
    unsigned long long seq_flag_seq = 0;            //   (their sequence numbers)
    int64_t ls_cap = 0, ls_tcap = 0, ls_rcap = 0;   // level-engine capacities grown on demand
    int64_t ls_hcap = 0, ls_fcap = 0;               //   and its two hash tables' slots (push, frontier)
    int32_t* pin_j = nullptr;                       // [P] index of link row L in inc(t) for each pin (t, L):
                                                    //   the level engine's pull levels (snapshot only, made on first use)
    int4* pull_rec = nullptr;                       // [I x 4] per incidence entry (t, L): L's <= 8 targets, then their
                                                    //   pin_j -- the pull walk's link data streamed in entry order
    int2* pull_meta = nullptr;                      // [I] (link atom, arity) per incidence entry
    int32_t pull_rec_state = 0;                     //   0 not built yet, 1 built, -1 over its memory budget
    int4* fc_rec = nullptr;                         // [I x 2] per incidence entry: its link's <= 8 targets (-1 padded),
    int32_t fc_rec_state = 0;                       //   the frontier-code pull's records (snapshot only, made on first
                                                    //   use; 0 not built, 1 built, -1 over budget / arity > 8)
    int32_t* fc_hubs = nullptr;                     //   and its hub atoms (ascending; their slots are in the records)
    int32_t fc_nhubs = 0;
    std::mutex seq_mu;                              // guards seq_hbufs (results hand their buffers back from any thread)
    std::vector<hgx::PoolBuf> seq_hbufs;            // mapped host buffers of order-exact results, free for reuse
    int32_t bfs_block = 1;                          // HGX_OPT_BFS_BLOCK: hgx_bfs_batch seeds first run one workgroup each
    // test / diagnostic options (hgx.h: HGX_OPT_CO_TIMEOUT .. HGX_OPT_XB_STATIC); 0 / -1 = the engine's default
    int64_t co_timeout = 0;                         // grid-stage barrier limit in s_memrealtime ticks (0 = 1 s)
    int32_t seq_pull = 1;                           // level engine pull levels: 0 never, 1 by width, 2 always
    int32_t seq_small = 0;                          // level engine: tiny starting capacities (exercise growth)
    int64_t seq_tlimit = 0;                         // level engine: stream-key limit below the 32-bit one (0 = none)
    int64_t seq_pack_min = 0;                       // level engine: pairs of a level that cross PCIe packed (0 = 2^20)
    int32_t xb_flat = -1, xb_static = -1;           // partition broadcast pack variants (-1 = default)
    int64_t sp_budget_bytes = (int64_t)48 << 30;    // HGX_OPT_SP_BUDGET (hgx_paths.h): shortest-path working arrays
    int32_t count_fused = 1;                        // HGX_OPT_COUNT_FUSED: dense-level kernels count the rows they store
    int32_t nf_pull = 1;                            // HGX_OPT_NF_PULL: 0 = late levels only, 8-entry step; 1 = the rule; 2 = every eligible level
    int32_t nf_hint = 1;                            // HGX_OPT_NF_HINT: direct-pull levels try the listed atoms' hint rows first
    int32_t hub_mask = 1;                           // HGX_OPT_HUB_MASK: 0 = off, 1 = the level rule, 2 = every eligible level;
    int32_t hub_mask_t = 32;                        //   atoms of the top list ORed into C (1 .. 64);
    uint32_t hub_mask_sched = 0x8Bu;                //   bit r: the hub pull tests its cover after round r of 256 entries
    unsigned long long* co_vis = nullptr;           // multi-workgroup stage: per-seed visited bitmaps (zero between calls)
    unsigned long long* sc_tab = nullptr;           // order-exact grid stage: level hash, word / key counts (empty between calls)
    int64_t co_vis_seeds = 0, co_pcap = 0;          //   seeds they hold; pair-list capacity (grown on demand)
    int64_t co_fr = 0;                              //   work items a level holds, all segments (likewise)
    int32_t co_ok = -1;                             //   its grid in blocks (0: does not fit; -1: not checked yet)
    int64_t co_timeouts = 0;                        //   launches whose grid barrier timed out (seeds fell back)
    int32_t sc_ok = -1;                             // order-exact grid stage (hgx_seq_coop): its grid (0: does not fit)
    int64_t sc_pcap = 0;                            //   its pair capacity (grown on demand)
    hgx_link_predicate* pred = nullptr;             // the link predicate of the traversal in progress (PredScope; under mu)
    const unsigned long long* sib = nullptr;        // the sibling predicate's bits of the traversal in progress (SibScope;
                                                    //   under mu): bit a set = atom a may be yielded; null = no predicate
    int64_t sib_fail = 0;                           //   and the atoms whose bit is 0
    std::deque<hgx::YieldList> ylists;              // yield lists (snapshot only; contexts read their base's)
    std::deque<hgx::YieldAdj> yadjs;                // yield adjacencies (likewise)
    std::mutex ylist_mu;
    // HGX_OPT_RANKS_ORDERED: rank order == persistent-handle order.  Cleared by an hgx_graph_update
    // that extends the rank space (appended ranks need not sort after the existing handles); the
    // order-exact traversal refuses to run until the caller re-asserts it.
    bool ranks_ordered = true;
    // Frontier-push accumulator rows (A x W words), all zero between levels: each push level ORs
    // into it and its finalise re-zeroes exactly the rows it consumed (no per-level clear).
    std::vector<int64_t> inc_off_host;   // host copy of inc_off (pattern planning), made on first use
    uint64_t* zacc = nullptr;
    unsigned long long* ctr_host = nullptr;   // push levels' counters, written by the finalise (mapped host memory)
    unsigned long long ctr_seq = 0;          // sequence numbers of those writes
    hipEvent_t pend_ev[2] = {nullptr, nullptr};   // the batched BFS's two in-flight level events
    uint64_t* hasinc = nullptr;          // [A/64 + 1] bit set <=> inc(atom) non-empty (non-full pull levels)
    int32_t* nbr_hint = nullptr;         // [A] the co-target of largest (degree, id) over the atom's links, -1 = none
                                         //   (HGX_OPT_NF_HINT: direct-pull levels, made on first use)
    int32_t* top_list = nullptr;         // [top_n <= 64] the atoms of largest (degree, id), descending
    int32_t top_n = 0;                   //   (HGX_OPT_HUB_MASK: dense levels, made on first use)
    uint8_t* inc_yf = nullptr;           // [I] ordered-mode yield flags per incidence (frontier push), made on first use
    hgx::HeavyChunk* pchunks = nullptr;  // frontier push: kPushChunk-entry chunks of atoms with deg > kPushLight
    int64_t n_pchunks = -1;              // -1 = not built yet
    size_t zacc_bytes = 0;
    bool zacc_clean = false;

    int64_t A = 0, M = 0, P = 0, I = 0;
    int32_t* link_atom = nullptr;
    int64_t* tgt_off = nullptr;
    int32_t* tgt_idx = nullptr;
    int32_t* link_type = nullptr;
    int64_t* inc_off = nullptr;
    int32_t* inc_row = nullptr;
    int32_t* inc_type = nullptr;    // [I] link_type[inc_row[i]]: streamed type filter of the query path
    // The optional type key of every atom (hgx_graph_set_atom_types, include/hgx_sibling.h): snapshot only, read
    // and replaced under the snapshot's mutex; type_preds = the living atom predicates evaluated from it.
    int32_t* atom_type = nullptr;   // [A]
    std::atomic<int> type_preds{0};
    // Type-grouped incidence (built on the first pattern query): inside each atom's segment the link
    // rows ordered by (type, row), so the links of one type incident to an atom are one contiguous,
    // ascending range (found by binary search over inc_ts_type).
    int32_t* inc_ts_row = nullptr;
    int32_t* inc_ts_type = nullptr;
    // Inline target rows of the type-grouped incidence (HGX_OPT_QUERY_INLINE, built with it): entry i
    // holds the <= 8 targets of link inc_ts_row[i] in 32 bytes (-1 padded; slot 0 = -2 for a link of
    // arity > 8, which the match reads through tgt_off).  A typed candidate then costs one streamed
    // 32-byte record instead of two dependent random rows.
    int32_t* inc_ts_tgt = nullptr;
    bool q_inline = true;
    // Type index of the links (hgx_scan.hip, built on the first scanned batch): one 16-byte record per link row,
    // (link atom, arity, first target offset low / high word), the rows stably sorted by link_type -- so the
    // links of one type are one segment, ascending by row and by atom.  type_key / type_seg: the sorted
    // distinct type keys and their segment offsets, on the host (a context copies its snapshot's).
    int4* type_idx = nullptr;
    bool type_idx_built = false;
    std::vector<int32_t> type_key;   // [n distinct types] ascending
    std::vector<int64_t> type_seg;   // [n distinct types + 1]
    // The atom index over atom_type (hgx_atoms.hip, built on the first use): the snapshot's is dropped with the
    // column; a context copies its snapshot's reference at every batch that scans.
    std::shared_ptr<hgx::AtomIndex> atom_index;

    int64_t n_heavy = 0;            // heavy atoms (deg > kHeavyDegree)
    int64_t I_heavy = 0;            // incidence entries of heavy atoms
    int64_t n_chunks = 0;
    int32_t* heavy_atom = nullptr;  // [n_heavy]
    hgx::HeavyChunk* chunks = nullptr;

    hgx::ShardInfo* shard = nullptr;   // set for a partition shard (hgx_shard_graph_create)

    std::vector<hgx::PoolBuf> pool;  // free device buffers for reuse across batches
    void* pinned = nullptr;          // small pinned host staging area
    size_t pinned_bytes = 0;
    void* mapped = nullptr;          // host-mapped result area the pattern kernels write into
    size_t mapped_bytes = 0;
    void* zc_in = nullptr;           // fine-grained pinned staging the pattern front kernel reads directly
    void* zc_in_dev = nullptr;       //   (its device address)
    size_t zc_in_bytes = 0;
    int64_t q_cap_chunks = 0, q_cap_cand = 0;   // pattern workspace capacity (grown on demand)
    int64_t q_hits_guess = 0;                   // result ids copied back with the head of the result area
    int32_t q_coalesce = 1;                     // HGX_OPT_QUERY_COALESCE: concurrent packed batches share device batches
    int64_t q_coalesce_max = 1 << 16;           //   at most this many queries per coalesced device batch
    hgx::QueryCombiner qcomb;
    unsigned long long* q_ticket = nullptr;     // pattern placement: blocks-done ticket (device, zero between batches)
    unsigned long long q_seq = 0;               //   sequence number of the completion flag in the result area

    void* alloc(size_t bytes);
    void release(void* p, size_t bytes);
    void* pinned_buf(size_t bytes);
    void* mapped_buf(size_t bytes);
    void* zc_in_buf(size_t bytes);   // host pointer; zc_in_dev is the kernels' view of it
};

// A link predicate (include/hgx_linkpred.h, hgx_linkpred.hip): its flags per link row and per incidence entry
// as int32 arrays, so that a traversal reads them in place of link_type / inc_type with the type key 1, and the
// per-(mode, type) lists the engines build over those arrays -- kept here, not on the snapshot, so they are keyed
// apart from every real type and every other predicate, and are freed with it.
struct hgx_link_predicate {
    hgx_graph* root = nullptr;       // the snapshot (a reference is held)
    std::atomic<int> refs{1};        // the caller's handle + one per result made with it
    int64_t M = 0, I = 0, n_sat = 0;
    int32_t* flag = nullptr;         // [M] 1 = the link row satisfies the predicate
    int32_t* inc_flag = nullptr;     // [I] flag[inc_row[i]]
    double ms_eval = 0, bytes_eval = 0;
    std::deque<hgx::YieldList> ylists;   // guarded by root->ylist_mu
    std::deque<hgx::YieldAdj> yadjs;
};

// A sibling predicate (include/hgx_sibling.h, hgx_sibling.hip): one bit an atom, 64 atoms to a word, the bits
// past the last atom zero.
struct hgx_atom_predicate {
    hgx_graph* root = nullptr;       // the snapshot (a reference is held)
    std::atomic<int> refs{1};        // the caller's handle + one per result made with it
    int64_t A = 0, n_kept = 0;
    unsigned long long* bits = nullptr;   // [A / 64 + 2]
    bool typed = false;              // evaluated from the snapshot's atom-type column (counted in root->type_preds)
    double ms_eval = 0, bytes_eval = 0;
};

namespace hgx {
// A reference for a result (p may be null) / dropping one: the last frees the arrays, the lists and the
// predicate's reference on its snapshot.  Neither needs a graph mutex.
inline hgx_link_predicate* pred_ref(hgx_link_predicate* p) {
    if (p) p->refs.fetch_add(1);
    return p;
}
void pred_release(hgx_link_predicate* p);
// The argument checks of the *_pred entry points (p not null): p belongs to g's snapshot, opts carries no type.
void pred_check(const hgx_graph* g, const hgx_link_predicate* p, const hgx_algen_opts* opts, const char* who);
// While alive, g's traversal code sees p's flags as link_type / inc_type and p's lists as the yield lists
// (p null: nothing changes).  The caller holds g->mu and passes the type key kLinkPredKey to the engines.
// Only code that holds g->mu may read g->link_type / g->inc_type (hgx_graph_context copies them under the
// snapshot's mutex; graph_release, which takes no lock, does not look at them for a context).
constexpr int32_t kLinkPredKey = 1;
struct PredScope {
    hgx_graph* g;
    int32_t *lt, *it;
    PredScope(hgx_graph* gg, hgx_link_predicate* p) : g(gg), lt(gg->link_type), it(gg->inc_type) {
        if (!p) return;
        g->link_type = p->flag;
        g->inc_type = p->inc_flag;
        g->pred = p;
    }
    ~PredScope() {
        g->link_type = lt;
        g->inc_type = it;
        g->pred = nullptr;
    }
    PredScope(const PredScope&) = delete;
    PredScope& operator=(const PredScope&) = delete;
};
// The same for a sibling predicate; apred_check: ap (not null) belongs to g's snapshot.
inline hgx_atom_predicate* apred_ref(hgx_atom_predicate* p) {
    if (p) p->refs.fetch_add(1);
    return p;
}
void apred_release(hgx_atom_predicate* p);
void apred_check(const hgx_graph* g, const hgx_atom_predicate* ap, const char* who);
// While alive, g's traversal code sees ap's bits in g->sib (ap null: nothing changes).  The caller holds g->mu.
struct SibScope {
    hgx_graph* g;
    SibScope(hgx_graph* gg, const hgx_atom_predicate* ap) : g(gg) {
        g->sib = ap ? ap->bits : nullptr;
        g->sib_fail = ap ? ap->A - ap->n_kept : 0;
    }
    ~SibScope() {
        g->sib = nullptr;
        g->sib_fail = 0;
    }
    SibScope(const SibScope&) = delete;
    SibScope& operator=(const SibScope&) = delete;
};
// The host checks of hgx_graph_set_atom_types over host copies of the link rows' atoms and types.
void atom_types_validate(int64_t A, int64_t M, const int32_t* atom_type, const int32_t* link_atom,
                         const int32_t* link_type);
// The batched BFS's sibling prologue (hgx_sibling.hip), enqueued on s after the seeds are written:
// every atom whose bit of keep is 0 gets vis row = fm (W words) and its ever / full bits.
void sib_saturate(const unsigned long long* keep, int64_t A, int W, const unsigned long long* fm,
                  unsigned long long* vis, unsigned long long* ever, unsigned long long* full, hipStream_t s);
// hgx_bfs_batch_sib / hgx_shortest_paths_sib behind the ABI's try block (hgx_bfs.hip, hgx_paths.hip); ap null:
// the _pred entry point.
void bfs_batch_sib(hgx_graph* g, const int32_t* seeds, int32_t n_seeds, int32_t max_depth, const hgx_algen_opts* opts,
                   hgx_link_predicate* p, hgx_atom_predicate* ap, hgx_bfs_result** out);
void shortest_paths_sib(hgx_graph* g, const int32_t* starts, const int32_t* goals, int32_t n_pairs,
                        const hgx_algen_opts* opts, const hgx_link_weights* w, hgx_link_predicate* p,
                        hgx_atom_predicate* ap, hgx_sp_result** out);
// The argument checks of hgx_bfs_result_sets (include/hgx_sets.h; hgx_sets.hip), all decided on the host: the
// statuses of the header's table, the messages naming the set.  n_result_seeds / shard: of the result asked.
void sets_validate(bool have_result, bool have_out, bool shard, int32_t n_result_seeds, const int32_t* seed_index,
                   int32_t n_sets, int32_t min_depth, int32_t max_depth, uint32_t flags);
void graph_release(hgx_graph* g);
void free_yield_lists(hgx_graph* g);   // (hgx_graph_update: the incidence changed)   // drop a reference; frees at zero
// Builds the BFS's first-use read-only tables (has-incidence bitmap, yield flags, push chunks) on g
// (hgx_bfs.hip; caller holds g->mu).
void bfs_shared_tables(hgx_graph* g);
// Upload + incidence build.  links_are_atoms = false for partition shards: link rows then carry
// their global link atom ids (not local atoms) and are not validated against num_atoms.
hgx_graph* graph_create(const hgx_graph_desc* d, int32_t device, bool links_are_atoms);
// Partitioned batched BFS over one shard; tr is the group's transport (hgx_bfs.hip).
void pbfs_run(hgx_graph* g, Transport* tr, const int32_t* seeds, int32_t n_seeds, int32_t max_depth,
              const hgx_algen_opts* opts, hgx_bfs_result** out);
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// Builds the ordered-mode yield flags (hgx_inc_yield, one byte per incidence entry + 64 bytes of
// padding for 16-byte vector loads) on g if absent; caller holds g->mu (hgx_bfs.hip).
void ensure_inc_yield(hgx_graph* g);
// Per (generator mode, link type): for each atom the links of its incidence entries of that type that
// can yield in that mode, in entry order (off [A + 1], row [n]); built on first use on the snapshot
// (shared by its contexts, freed with it).  nullptr for the symmetric mode without a type (the
// incidence itself) and once kMaxYieldLists lists exist.  Caller holds g->mu (hgx_seq.hip).
const YieldList* yield_list(hgx_graph* g, int mode, int32_t type);
// The generator's (target, link atom) output per atom for (mode, type, minimum arity, reverse order),
// in stream order; built on first use on the snapshot.  nullptr for the symmetric mode without a type,
// when refused (over kYieldAdjBudget) and once kMaxYieldLists exist.  Caller holds g->mu (hgx_seq.hip).
const YieldAdj* yield_adj(hgx_graph* g, int mode, int32_t type, int32_t min_arity, bool rev);
// The set-mode workgroup engine's part of one hgx_bfs_batch (hgx_seq.hip, HGX_OPT_BFS_BLOCK): per seed
// V_1, V_2, ... one after the other (atoms) and |V_d| (lcnt[d - 1]) in mapped host buffers the
// result owns; the seeds whose traversal outgrew a workgroup are listed in rerun (the batched engine
// runs them).
struct BlockSet {
    std::vector<PoolBuf> bufs;
    std::vector<int32_t> seeds;                 // [n seeds] the start atoms (V_0)
    std::vector<const int32_t*> atoms, lcnt;   // [n seeds] (nullptr: rerun)
    std::vector<int32_t> pairs, levels;         // [n seeds] atoms past V_0 (-1: rerun), levels with news
    std::vector<int32_t> rerun;                 // seed indices, ascending
    double traversed = 0, ms = 0, bytes = 0;   // items of the finished seeds; device ms; algorithmic bytes
    int32_t expanded = 0;                       // most levels expanded by one finished seed
    // Seeds the multi-workgroup stage finished (the workgroup stage's overflow, <= kMaxCoSeeds of
    // them): their (atom, seed | level << 8) pairs stay in device pool memory until a reader asks for
    // a set (block_materialize); their level counts are on the host at once.
    void* co_pairs = nullptr;                   // kCoSegs segments of co_pseg pairs, co_segn[q] used in q
    size_t co_bytes = 0;
    int64_t co_n = 0, co_pseg = 0;
    std::vector<int64_t> co_segn;
    std::vector<int32_t> co_idx;                // seed indices
    std::vector<std::vector<int32_t>> co_lcnt, co_atoms;
    bool co_host = false;
    double co_ms = 0, co_bytes_alg = 0;         // device ms of that launch (timing on), its algorithmic bytes
    int32_t n_coop = 0;                         // seeds it finished
    int32_t co_fallbacks = 0;                   // its launches that timed out on a grid barrier (rows engine ran)
};
constexpr int kMaxCoSeeds = 64;
// Runs every seed on the workgroup engine (caller holds g->mu, g's device current; max_depth -1 =
// unbounded); returns when the seeds are done.
void bfs_block(hgx_graph* g, const int32_t* seeds, int32_t n_seeds, int32_t max_depth, const hgx_algen_opts& o,
               BlockSet& out);
// Hands the result's mapped buffers back to the graph's pool (caller holds g->mu).
void block_release(hgx_graph* g, BlockSet& b);
// Per-seed atom lists of the multi-workgroup stage's seeds on the host (first reader; g->mu held).
void block_materialize(hgx_graph* g, BlockSet& b);
// Waits for the work enqueued on s by polling: hipStreamSynchronize sleeps and wakes tens of
// microseconds after the last kernel, a cost per call of the short pattern batches.
inline void spin_sync(hipStream_t s) {
    hipError_t e;
    while ((e = hipStreamQuery(s)) == hipErrorNotReady) {
    }
    HGX_HIP(e);
}
// As spin_sync for one event (the blocking wait adds tens of microseconds per BFS level, and unbounded
// traversals run tens of short levels).
inline void spin_event(hipEvent_t ev) {
    hipError_t e;
    while ((e = hipEventQuery(ev)) == hipErrorNotReady) {
    }
    HGX_HIP(e);
}
// Waits for a word of mapped host memory that a kernel on s stores `want` into, by polling.  The stream is
// asked every 1024 polls: one that finished or failed without the word is an error (HGX_E_DEVICE, `what`).
inline void wait_host_word(const u64* word, u64 want, hipStream_t s, const char* what) {
    for (unsigned spin = 0; __atomic_load_n(word, __ATOMIC_ACQUIRE) != want; ++spin) {
        if ((spin & 1023u) != 1023u) continue;
        const hipError_t e = hipStreamQuery(s);
        if (e == hipErrorNotReady) continue;
        if (e != hipSuccess) HGX_HIP(e);
        if (__atomic_load_n(word, __ATOMIC_ACQUIRE) != want) fail(HGX_E_DEVICE, what);
    }
}
// Device buffers of one call or one batch from the graph's pool, given back at scope exit (an error path
// included; the caller holds g->mu).  Releasing into the pool is stream-ordered: no synchronisation.
struct PoolScratch {
    hgx_graph* g;
    std::vector<std::pair<void*, size_t>> t;
    void* take(size_t bytes) {
        t.emplace_back(nullptr, bytes);   // the slot first: a failed allocation of either kind strands nothing
        return t.back().first = g->alloc(bytes);
    }
    void give_back() {   // now, and the object is empty again (its capacity stays)
        for (auto& x : t)
            if (x.first) g->release(x.first, x.second);
        t.clear();
    }
    ~PoolScratch() { give_back(); }
};
// The generator's closed-form neighbour rule as a mode (every engine's kernels switch on it).
enum Mode { kSym = 0, kAfterFirst = 1, kBeforeFirst = 2, kBeforeLast = 3, kAfterLast = 4 };
// Mirrors pyref.mode_of (validated exhaustively against the DefaultALGenerator restatement).
inline int mode_of(const hgx_algen_opts& o) {
    bool P = o.return_preceding, S = o.return_succeeding, R = o.reverse_order, RS = o.return_source;
    if (!R) {
        if (!P) return kAfterFirst;
        if (!S && !RS) return kBeforeFirst;
        return kSym;
    }
    if (!P) return kBeforeLast;
    if (!S && !RS) return kAfterLast;
    return kSym;
}
inline int grid_for(int64_t work_items, int block, int max_blocks = 8192) {
    int64_t b = ceil_div(work_items > 0 ? work_items : 1, block);
    return (int)(b < max_blocks ? b : max_blocks);
}
// The union stage of a DNF batch (hgx_union.hip) over the clause results the pattern
// pipeline left in device memory.  Everything but the out_* pointers (the mapped result area) is device
// memory; ctr is zeroed by the launcher.
struct UnionArgs {
    int32_t n_queries, n_clauses;
    const int64_t* clause_off;   // [n_queries + 1] clauses of each query
    const int64_t* run_off;      // [n_clauses + 1] hit offsets of each clause (hgx_q_place's result offsets)
    const int32_t* hits;         // [cap] the clause hits, each clause ascending
    int64_t cap;                 // workspace capacity in hits (the grids and the scan are sized from it)
    const int64_t* stat;         // [8] statistics of the clause stage: [2] overflow
    uint8_t* keep;               // [cap + 1] keep flags
    int64_t* pre;                // [cap + 1] their exclusive prefix sum
    void* tmp;                   // scan temporary storage (union_temp_bytes)
    size_t tmp_bytes;
    unsigned long long* ctr;     // [4] binary-search probes / runs visited of keep, of place
    int64_t* out_stat;           // [8] mapped: the clause stage's statistics, [3] ids kept, [6] clause hits
    unsigned long long* out_ctr; // [4] mapped: ctr
    int64_t* out_off;            // [n_queries + 1] mapped: result offsets
    int32_t* out_ids;            // [cap] mapped: result ids
};
size_t union_temp_bytes(int64_t cap, hipStream_t s);
// Enqueues the union on s: no synchronisation, nothing read back by the host.
void union_launch(const UnionArgs& a, hipStream_t s);

// The join stage of a join batch (hgx_pattern_batch_join, include/hgx_join.h; hgx_join.hip)
// behind the union, which then leaves its offsets and ids in device memory: the "queries" of the union are the
// parts of the join queries.  Everything but the out_* pointers (the mapped result area) is device memory; ctr
// is zeroed by the launcher.  keep / pre / tmp may be the union's (it is done with them).
struct JoinArgs {
    int32_t n_queries, n_parts;
    const int64_t* part_off;     // [n_queries + 1] parts of each join query
    const int32_t* part_pos;     // [n_parts] target position of each part, HGX_JOIN_SELF = the link atom
    const int64_t* uoff;         // [n_parts + 1] the union's result offsets (one result per part)
    const int32_t* uids;         // [cap] the union's result ids (link atoms)
    int64_t cap;                 // workspace capacity in hits (the grids, the sort and the scan are sized from it)
    const int64_t* stat;         // [8] statistics of the clause stage: [2] overflow
    int64_t M;                   // the snapshot's link rows
    const int32_t* link_atom;
    const int64_t* tgt_off;
    const int32_t* tgt_idx;
    u64* key;                    // [cap] (part << 32) | value; past the hits a pad key that sorts last
    u64* key_sorted;             // [cap]
    int32_t sort_bits;           // the sort covers the low 32 + bits(n_parts) bits
    void* sort_tmp;              // radix sort temporary storage (join_temp_bytes)
    size_t sort_tmp_bytes;
    uint8_t* keep;               // [cap + 1] keep flags of the sorted keys
    int64_t* pre;                // [cap + 1] their exclusive prefix sum
    void* tmp;                   // scan temporary storage (union_temp_bytes)
    size_t tmp_bytes;
    unsigned long long* ctr;     // [8] hits projected, distinct values, -, key probes, keep probes, targets read
    unsigned long long* out_ctr; // [8] mapped: ctr, [2] = ids kept
    int64_t* out_off;            // [n_queries + 1] mapped: result offsets
    int32_t* out_ids;            // [cap] mapped: result ids (atoms)
    // hgx_pattern_batch_atoms: the bits of each join query's atom predicate (a null entry: none), or null: a batch
    // without predicates, which runs the keep kernel without the filter.  ctr[6] / [7]: values tested / rejected.
    const unsigned long long* const* keep_bits;   // [n_queries]
};
// Bits of the part field of a key: enough for the pad key's part, n_parts.
inline int32_t join_part_bits(int64_t n_parts) {
    int32_t b = 1;
    while (b < 31 && ((int64_t)1 << b) <= n_parts) ++b;
    return b;
}
size_t join_temp_bytes(int64_t cap, int32_t sort_bits, hipStream_t s);
// Enqueues the join on s: no synchronisation, nothing read back by the host.  k0 / k1 (both or neither): events
// recorded around the keep kernel.
void join_launch(const JoinArgs& a, hipStream_t s, hipEvent_t k0 = nullptr, hipEvent_t k1 = nullptr);
// The host checks of the join arrays (hgx_join.hip): HGX_E_INVALID naming the join query and the part.  who: the
// entry point's name; known_flags: the flag bits it takes.
void join_validate(int32_t n_queries, const int64_t* part_off, const int32_t* part_pos, int32_t flags,
                   const char* who = "hgx_pattern_batch_join", int32_t known_flags = HGX_JOIN_TYPE_SCAN);
// The host checks of hgx_pattern_batch_atoms's keep table (hgx_atoms.hip): every predicate belongs to g's
// snapshot, else HGX_E_INVALID naming the join query.  Returns the queries that carry one.
int64_t atoms_keep_validate(const hgx_graph* g, int32_t n_queries, hgx_atom_predicate* const* keep);
// HGX_E_UNSUPPORTED (who names the entry point) unless g's snapshot has an atom-type column; takes the snapshot's
// mutex, so the caller holds none.
void atoms_require_types(hgx_graph* g, const char* who);

// The negation program of a DNF batch (hgx_pattern_batch_dnf_not, include/hgx_not.h) as the caller handed
// it over; not_validate fills the totals.
struct NotProgram {
    const int64_t* neg_off = nullptr;    // [n_clauses + 1]
    const int64_t* term_off = nullptr;   // [n_negs + 1]
    const int64_t* lit_off = nullptr;    // [n_terms + 1]
    const int32_t* lit = nullptr;        // [4 n_lits] (kind, polarity, op_beg, op_end)
    const int32_t* ops = nullptr;        // [n_ops]
    int64_t n_ops = 0, n_negs = 0, n_terms = 0, n_lits = 0;
};
// Every offset, operand range, atom id and kind of the program, on the host (hgx_not.hip): fails with
// HGX_E_INVALID / HGX_E_UNSUPPORTED naming the query, the clause and the negation.  A = atoms of the graph.
void not_validate(int64_t A, int32_t n_queries, const int64_t* clause_off, NotProgram& p);
// The checks of literal l alone (operand range, operand count, atom ids, kind, limits): 0, or the status with the
// reason in why -- the caller puts the place in front of it.  Shared by not_validate and linkpred_validate.
int not_check_literal(int64_t A, const NotProgram& p, int64_t l, std::string& why);
// The same checks for a link predicate (include/hgx_linkpred.h): one tree in disjunctive normal form, n_terms
// terms; fills p.n_terms / p.n_lits and tells whether a literal reads targets.  Messages name the term and the
// literal.
void linkpred_validate(int64_t A, int64_t n_terms, NotProgram& p, bool* needs_targets);
// The host checks of hgx_atom_predicate_create's program (hgx_sibling.hip): those of linkpred_validate, and
// HGX_E_UNSUPPORTED for a literal that is no HGX_NOT_TYPE.  Fills p.n_terms / p.n_lits.
void atompred_validate(int64_t A, int64_t n_terms, NotProgram& p);
// Its device copy (neg_off == nullptr: the batch has no negation).
struct NotDev {
    const int64_t* neg_off = nullptr;
    const int64_t* term_off = nullptr;
    const int64_t* lit_off = nullptr;
    const int4* lit = nullptr;
    const int32_t* ops = nullptr;
};
// The filter stage of a DNF batch with negations (hgx_not.hip), between the clause stage and
// the union: the clause hits that pass their clause's negations, compacted into hits_out / run_out in the
// layout the union reads.  flag / pre / tmp are the union's keep / pre / tmp (it overwrites them afterwards).
struct NotArgs {
    NotDev prog;
    int32_t n_clauses;
    const int64_t* run_off;      // [n_clauses + 1] hit offsets of each clause
    const int32_t* hits;         // [cap] the clause hits (link atoms)
    int64_t cap;
    const int64_t* stat;         // [8] statistics of the clause stage: [2] overflow
    int64_t M;                   // the snapshot's link rows
    const int32_t* link_atom;
    const int64_t* tgt_off;
    const int32_t* tgt_idx;
    const int32_t* link_type;
    uint8_t* flag;               // [cap + 1] 1 = the hit passes
    int64_t* pre;                // [cap + 1] exclusive prefix sum of flag
    void* tmp;                   // scan temporary storage (union_temp_bytes)
    size_t tmp_bytes;
    int32_t* hits_out;           // [cap] the hits that pass, each clause ascending
    int64_t* run_out;            // [n_clauses + 1] their offsets
    unsigned long long* ctr;     // [8] tested, rejected, targets read, types read, row-search probes
    unsigned long long* out_ctr; // [8] mapped: ctr
};
// Enqueues the filter on s: no synchronisation, nothing read back by the host.
void not_launch(const NotArgs& a, hipStream_t s);
}  // namespace hgx

namespace hgx {
// The type index of g's links, built on first use (hgx_scan.hip; caller holds g->mu, g's device current).  A
// context takes its snapshot's (built there under the snapshot's mutex).
void ensure_type_index(hgx_graph* g);
// hgx_graph_update: the links changed, the next scan rebuilds the index.
void drop_type_index(hgx_graph* g);

// One scanned clause of a DNF batch (hgx_pattern_batch_dnf_scan): a clause without an incidence anchor and
// with exactly one type, evaluated over the type's segment of the index.
struct ScanDesc {
    int64_t seg_beg, seg_len;   // the type's segment of the index (seg_len 0: absent type or a NOP clause)
    int64_t g0, g1;             // its negations in the program
    int32_t clause;             // its index among the batch's clauses
    int32_t type;               // its type key (a type literal of its negations compares with this)
    int32_t arity;              // arity == k, or -1
    int32_t min_arity;          // longest all-ANY ordered pattern (arity >= m)
    int32_t needs_targets;      // a literal of its negations reads targets
    int32_t pad;
};
// The scan stage of a DNF batch (hgx_scan.hip), between the clause stage (+ filter) and the
// union: the hits of the scanned clauses, merged with the anchored clauses' runs into hits_out / run_out in
// the layout the union reads.
struct ScanArgs {
    NotDev prog;
    int32_t n_scan, n_clauses;
    int64_t n_chunks;               // 64-entry chunks over every scanned clause (> 0)
    const ScanDesc* desc;           // [n_scan]
    const int64_t* chunk_beg;       // [n_scan + 1] first chunk of each scanned clause
    const int64_t* clause_chunk;    // [n_clauses + 1] chunks of the scanned clauses before clause c
    const int4* idx;                // the type index
    const int32_t* tgt_idx;
    u64* word;                      // [n_chunks] keep bits of the chunk's lanes
    int64_t* cnt;                   // [n_chunks + 1] their population counts (last: 0)
    int64_t* cpre;                  // [n_chunks + 1] exclusive prefix sum of cnt
    void* tmp;                      // scan temporary storage (scan_temp_bytes)
    size_t tmp_bytes;
    int64_t* stat;                  // [8] statistics of the clause stage: [1] needed capacity, [2] overflow
    const int64_t* run_in;          // [n_clauses + 1] hit offsets of the clause stage (scanned clauses: empty runs)
    const int32_t* hits_in;         // [cap] its hits
    int64_t cap;
    bool move;                      // the batch has an anchored clause: its hits move to their merged places
    int64_t* run_out;               // [n_clauses + 1] merged hit offsets
    int32_t* hits_out;              // [cap] merged hits, each clause ascending
    unsigned long long* ctr;        // [8] rows kept, targets read, rows that walked a program
    unsigned long long* out_ctr;    // [8] mapped: ctr
};
size_t scan_temp_bytes(int64_t n_chunks, hipStream_t s);
// Enqueues the scan stage on s: no synchronisation, nothing read back by the host.  atoms: a.idx is the atom index
// (hgx_atoms.hip), whose node records take the node rules of include/hgx_atoms.h.
void scan_launch(const ScanArgs& a, hipStream_t s, bool atoms = false);
// The atom index of g's snapshot, built on first use (hgx_atoms.hip; caller holds g->mu, g's device current; a
// context takes its snapshot's under the snapshot's mutex).  HGX_E_UNSUPPORTED (who names the entry point): no
// atom-type column.
std::shared_ptr<AtomIndex> ensure_atom_index(hgx_graph* g, const char* who);
}  // namespace hgx

// One batch (<= 1024 seeds) of a batched BFS and the result object of hgx_bfs_batch (hgx_bfs.hip makes and
// frees them; hgx_hops.hip reads the level rows).
struct BfsBatch {
    int32_t seed0 = 0, S = 0, W = 0;
    int32_t n_expanded = 0;       // levels whose frontier was expanded (advance() iterated)
    std::vector<hgx::u64*> lvl;   // per level, A*W words (rows valid where fa bit set)
    std::vector<hgx::u64*> fa;    // per level, A bits
    hgx::u64* pcnt = nullptr;     // [kDirectLevels][1024] per-source counts of push levels (whole graph)
    std::vector<char> direct;     // direct[d]: level d's counts are in pcnt (no counting pass)
    // Levels counted before the readout: cpart[d] = level d's block partials, cblk[d] blocks of W*64
    // words (null = counted at readout).  Written by the kernels that stored the level's rows (fused
    // counts, HGX_OPT_COUNT_FUSED) or by a counting pass launched on g->stream2 next to the following
    // levels (HGX_COUNT_EAGER, A/B).
    std::vector<uint32_t*> cpart;
    std::vector<int32_t> cblk;
    void set_cpart(size_t lev, uint32_t* p, int32_t blocks) {
        if (cpart.size() <= lev) {
            cpart.resize(lev + 1, nullptr);
            cblk.resize(lev + 1, 0);
        }
        cpart[lev] = p;
        cblk[lev] = blocks;
    }
    size_t cpart_bytes(size_t lev) const { return sizeof(uint32_t) * (size_t)cblk[lev] * W * 64; }
    int32_t pass_levels = 0;      // levels the readout still has to count with a pass over their rows
};

struct hgx_bfs_result {
    hgx_graph* g = nullptr;
    int32_t n_seeds = 0, n_levels = 0;
    std::vector<BfsBatch> batches;
    hgx_bfs_stats stats{};
    bool counts_ready = false, accounting_ready = false;
    bool typed = false;
    hgx_algen_opts opts{HGX_NO_TYPE, 1, 1, 0, 0};   // the generator the result was made with (hgx_hops.h readers)
    hgx_link_predicate* pred = nullptr;             // its link predicate (a reference; opts.link_type is then kLinkPredKey)
    hgx_atom_predicate* apred = nullptr;            // its sibling predicate (a reference, kept for the lifetime rule only:
                                                    //   the level rows already leave out the atoms that fail it)
    std::map<int32_t, int32_t> isolated;   // shards: seed index -> owned seed atom without incidence
    std::vector<int64_t> counts;   // [n_seeds * n_levels]
    // Seeds finished by the workgroup engine (HGX_OPT_BFS_BLOCK); the batches then hold only the
    // others, compacted: orig[k] = seed index of batch seed k, compact[i] = k (-1: a workgroup seed).
    std::unique_ptr<hgx::BlockSet> blk;
    std::vector<int32_t> orig, compact;
    // hgx_hops.h row readers: the depth and predecessor-key rows of one seed, kept until the result is freed
    // (12 A bytes of pool memory; hop_seed = the seed index they belong to, hop_have_key = the key row is filled).
    int32_t hop_seed = -1;
    bool hop_have_key = false;
    int32_t* hop_depth = nullptr;   // [A]
    hgx::u64* hop_key = nullptr;    // [A] (predecessor atom << 32) | link atom
    int32_t orig_of(int32_t k) const { return orig.empty() ? k : orig[k]; }
    size_t row_bytes(const BfsBatch& b) const { return sizeof(hgx::u64) * (size_t)g->A * b.W; }
    size_t bm_bytes() const { return sizeof(hgx::u64) * (size_t)(g->A / 64 + 2); }
};
