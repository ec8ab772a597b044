// directional.hip — count-aware ("directional") UMI clustering on gfx950.
//
// Vertices are the distinct regular strings (byte length L, only ACGT, L 1..32) as 2-bit
// codes, first base in the highest digit, each with count = its rows. There is a directed
// edge a -> b when the codes differ in exactly one digit and count(a) >= 2 count(b) - 1.
// root(v) is the vertex of largest key (count, then the smaller code) among all vertices
// that reach v, v included; a cluster is the set of vertices sharing a root. Irregular
// strings take no edges and are grouped by exact bytes (irregular.hip), after the regular
// clusters.
//
//   count   the shared front end (sorted_codes.hip): the regular rows sorted by code, the
//           sorted distinct codes D[m], their counts C[m] and every sorted row's index
//           into D.
//   edges   one lane per distinct code v probes its 3 L one-substitution neighbours in D
//           by binary search (two distinct integers d apart in value are at most d apart
//           in a sorted array of distinct integers, which bounds the search window: the
//           low digits need 2-4 steps) and keeps the in-neighbours u that pass the count
//           test, adj[k * m + v] = u for k < deg[v]. Stored once; the rounds do not
//           search again. The table is 3 L columns of m entries, so lanes read it
//           coalesced, and one search pass fills it (a compacted CSR needs a second one).
//   relax   best[v] = max(best[v], best[u] over in-neighbours u, best[root of best[v]]),
//           on the u64 key count << 32 | (0xFFFFFFFF - index in D): D ascends, so the
//           smaller index is the smaller code. In place: the update is monotone and every
//           value a lane can read is the key of an ancestor, so a stale read only delays
//           a round and the fixed point is the same however lanes interleave. A round that
//           improves nothing ends the loop (directional_rounds.h).
//   label   flag best[v] == key(v), scan in D order, labels[v] = rank of v's root.
#include <hipcub/hipcub.hpp>

#include "column_util.h"
#include "level2.h"
#include "directional_rounds.h"

namespace rogtk {
namespace {

constexpr int kBlock = 256;
constexpr int kCtrlWords = 64;  // [0, kDirBatch): changed words; [8]: cluster count

// ------------------------------------------------------------------- edges
__device__ __forceinline__ unsigned long long dir_key(uint32_t count, uint32_t v) {
    return ((unsigned long long)count << 32) | (unsigned long long)(0xFFFFFFFFu - v);
}
__device__ __forceinline__ uint32_t dir_index(unsigned long long key) { return 0xFFFFFFFFu - (uint32_t)key; }

// WINDOW: D holds composites key << shift | code. A substitution changes the
// low digits alone, so a neighbour lies among the entries of the lane's own key, [gb, ge):
// kWindowTable reads that range from the table of key heads, kWindowGallop finds it by
// doubling steps out from v and a binary search of the last step. The value bound below is
// then clamped to it: for the high digits it is the whole array otherwise. kWindowValue is
// the ungrouped kernel, unchanged.
template <int WINDOW>
__global__ void __launch_bounds__(kBlock)
k_dir_edges(const uint64_t* __restrict__ D, const uint32_t* __restrict__ C, int64_t m, int L,
            uint32_t* __restrict__ deg, uint32_t* __restrict__ adj, unsigned long long* __restrict__ best,
            int shift, const uint32_t* __restrict__ gidx, const uint32_t* __restrict__ gstart) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= m) return;
    const uint64_t code = D[v];
    const uint32_t cv = C[v];
    const uint64_t need = 2ull * (uint64_t)cv - 1ull;  // count(u) >= 2 count(v) - 1, in 64 bits
    uint32_t nd = 0;
    [[maybe_unused]] int64_t gb = 0, ge = m;
    if constexpr (WINDOW == kWindowTable) {
        const uint32_t g = gidx[v];
        gb = gstart[g];
        ge = gstart[g + 1];
    } else if constexpr (WINDOW == kWindowGallop) {
        if (shift < 64) {
            const uint64_t first = (code >> shift) << shift;      // the key's smallest composite
            const uint64_t last = first | ((1ull << shift) - 1);  // and its largest
            int64_t step = 1, hi = v;                             // D[hi] >= first
            while (hi - step >= 0 && D[hi - step] >= first) {
                hi -= step;
                step <<= 1;
            }
            int64_t lo = hi - step >= 0 ? hi - step + 1 : 0;  // D[lo - 1] < first (or lo == 0)
            while (lo < hi) {                                 // first index with D[index] >= first
                const int64_t mid = (lo + hi) >> 1;
                if (D[mid] < first) lo = mid + 1;
                else hi = mid;
            }
            gb = lo;
            step = 1;
            lo = v;  // D[lo] <= last
            while (lo + step < m && D[lo + step] <= last) {
                lo += step;
                step <<= 1;
            }
            hi = lo + step < m ? lo + step : m;  // D[hi] > last (or hi == m)
            ++lo;
            while (lo < hi) {  // first index with D[index] > last
                const int64_t mid = (lo + hi) >> 1;
                if (D[mid] <= last) lo = mid + 1;
                else hi = mid;
            }
            ge = lo;
        }
    }
    for (int p = 0; p < L; ++p) {
        for (uint64_t x = 1; x <= 3; ++x) {
            const uint64_t q = code ^ (x << (2 * p));
            // |index(q) - v| <= |q - code|: the codes between them are distinct integers
            int64_t lo, hi;
            if (q < code) {
                const uint64_t d = code - q;
                lo = d < (uint64_t)v ? v - (int64_t)d : 0;
                hi = v;
            } else {
                const uint64_t d = q - code;
                lo = v + 1;
                hi = d < (uint64_t)(m - v) ? v + (int64_t)d + 1 : m;
            }
            if constexpr (WINDOW != kWindowValue) {
                lo = max(lo, gb);
                hi = min(hi, ge);
            }
            while (lo < hi) {  // first index in [lo, hi) with D[index] >= q
                const int64_t mid = (lo + hi) >> 1;
                if (D[mid] < q) lo = mid + 1;
                else hi = mid;
            }
            if (lo < (WINDOW != kWindowValue ? ge : m) && D[lo] == q && (uint64_t)C[lo] >= need) {
                adj[(int64_t)nd * m + v] = (uint32_t)lo;
                ++nd;
            }
        }
    }
    deg[v] = nd;
    best[v] = dir_key(cv, (uint32_t)v);
}

// ------------------------------------------------------------------- relax
// One round, in place. best[] is read and written by other workgroups in the same launch:
// relaxed agent-scope accesses keep each 8-byte key whole, and any value read, however
// stale, is the key of an ancestor (see the header comment), so no ordering is needed.
__device__ __forceinline__ unsigned long long best_load(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ void __launch_bounds__(kBlock)
k_dir_relax(const uint32_t* __restrict__ deg, const uint32_t* __restrict__ adj, int64_t m,
            unsigned long long* best, uint32_t* changed) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool moved = false;
    if (v < m) {
        const unsigned long long old = best_load(best + v);
        unsigned long long b = old;
        const uint32_t nd = deg[v];
        for (uint32_t k = 0; k < nd; ++k) b = max(b, best_load(best + adj[(int64_t)k * m + v]));
        b = max(b, best_load(best + dir_index(b)));  // an ancestor's ancestor is an ancestor
        if (b != old) {
            __hip_atomic_store(best + v, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            moved = true;
        }
    }
    if (__ballot(moved) && (threadIdx.x & 63) == 0) *changed = 1u;
}

// ------------------------------------------------------------------- label
__global__ void k_dir_roots(const unsigned long long* __restrict__ best, int64_t m, uint32_t* __restrict__ root,
                            uint32_t* __restrict__ flag) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= m) return;
    const uint32_t r = dir_index(best[v]);
    root[v] = r;
    flag[v] = r == (uint32_t)v;
}

__global__ void k_dir_labels(const uint32_t* __restrict__ root, const uint32_t* __restrict__ flag,
                             const uint32_t* __restrict__ rank, int64_t m, uint32_t* __restrict__ labels,
                             uint32_t* __restrict__ total) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= m) return;
    labels[v] = rank[root[v]];
    if (v == m - 1) *total = rank[v] + flag[v];
}

// every sorted regular row: the label (and the root's code) of its distinct code
__global__ void k_dir_rows(const uint32_t* __restrict__ row, const uint32_t* __restrict__ idx, int64_t n,
                           const uint32_t* __restrict__ labels, const uint32_t* __restrict__ root,
                           const uint64_t* __restrict__ D, uint32_t* __restrict__ cluster_id,
                           uint64_t* __restrict__ root_code) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n) return;
    const uint32_t j = idx[k], i = row[k];
    cluster_id[i] = labels[j];
    if (root_code) root_code[i] = D[root[j]];
}

__global__ void k_dir_stats(int64_t* stats, int64_t n_regular_clusters) {
    stats[0] = 0;
    stats[1] = n_regular_clusters;
}

struct CodesLayout {
    size_t off_ctrl, off_best, off_deg, off_flag, off_rank, off_adj, off_scan, scan_bytes, total;
};

int codes_layout(int64_t m, int L, CodesLayout* p) {
    const int64_t m1 = std::max<int64_t>(m, 1);
    size_t sb = 0;
    ROGTK_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, sb, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                     (int)m1));
    Carve c;
    p->off_ctrl = c.take(kCtrlWords * 4);
    p->off_best = c.take((size_t)m1 * 8);
    p->off_deg = c.take((size_t)m1 * 4);
    p->off_flag = c.take((size_t)m1 * 4);
    p->off_rank = c.take((size_t)m1 * 4);
    p->off_adj = c.take((size_t)m1 * 4 * (size_t)(3 * L));
    p->scan_bytes = sb;
    p->off_scan = c.take(sb);
    p->total = c.total;
    return ROGTK_OK;
}

}  // namespace

int directional_codes_temp(int64_t m, int L, int64_t* bytes) {
    CodesLayout p;
    if (int rc = codes_layout(m, L, &p)) return rc;
    *bytes = (int64_t)p.total;
    return ROGTK_OK;
}

int directional_codes(const uint64_t* D, const uint32_t* C, int64_t m, int L, uint32_t* root, uint32_t* labels,
                      int64_t* n_clusters, int64_t* rounds, void* temp, int64_t temp_bytes, hipStream_t s,
                      const DirGroups* grp) {
    *n_clusters = 0;
    *rounds = 0;
    if (m <= 0) return ROGTK_OK;
    CodesLayout p;
    if (int rc = codes_layout(m, L, &p)) return rc;
    ROGTK_REQUIRE((int64_t)p.total <= temp_bytes, ROGTK_E_INVALID, "directional: temp_bytes %lld too small (need %lld)",
                  (long long)temp_bytes, (long long)p.total);
    uint8_t* t = (uint8_t*)temp;
    uint32_t* ctrl = (uint32_t*)(t + p.off_ctrl);
    unsigned long long* best = (unsigned long long*)(t + p.off_best);
    uint32_t* deg = (uint32_t*)(t + p.off_deg);
    uint32_t* flag = (uint32_t*)(t + p.off_flag);
    uint32_t* rank = (uint32_t*)(t + p.off_rank);
    uint32_t* adj = (uint32_t*)(t + p.off_adj);
    const dim3 g(grid_for(m, kBlock)), b(kBlock);
    const uint32_t* no_table = nullptr;
    if (grp && grp->window == kWindowTable)
        hipLaunchKernelGGL(k_dir_edges<kWindowTable>, g, b, 0, s, D, C, m, L, deg, adj, best, grp->shift, grp->gidx,
                           grp->gstart);
    else if (grp && grp->window == kWindowGallop)
        hipLaunchKernelGGL(k_dir_edges<kWindowGallop>, g, b, 0, s, D, C, m, L, deg, adj, best, grp->shift, no_table,
                           no_table);
    else
        hipLaunchKernelGGL(k_dir_edges<kWindowValue>, g, b, 0, s, D, C, m, L, deg, adj, best, 0, no_table, no_table);
    ROGTK_HIP_CHECK(hipGetLastError());
    auto launch = [&](int64_t, int k) -> int {
        ROGTK_HIP_CHECK(hipMemsetAsync(ctrl, 0, 16, s));
        for (int j = 0; j < k; ++j) hipLaunchKernelGGL(k_dir_relax, g, b, 0, s, deg, adj, m, best, ctrl + j);
        ROGTK_HIP_CHECK(hipGetLastError());
        return ROGTK_OK;
    };
    auto read = [&](int k, uint32_t* changed) -> int {
        ROGTK_HIP_CHECK(hipMemcpyAsync(changed, ctrl, (size_t)k * 4, hipMemcpyDeviceToHost, s));
        ROGTK_HIP_CHECK(hipStreamSynchronize(s));
        return ROGTK_OK;
    };
    const int rc = directional_run_rounds(m, launch, read, rounds);
    if (rc > 0) return rc;
    ROGTK_REQUIRE(rc == 0, ROGTK_E_HIP, "directional: no fixed point after %lld rounds over %lld codes",
                  (long long)*rounds, (long long)m);
    hipLaunchKernelGGL(k_dir_roots, g, b, 0, s, best, m, root, flag);
    size_t sb = p.scan_bytes;
    ROGTK_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(t + p.off_scan, sb, flag, rank, (int)m, s));
    hipLaunchKernelGGL(k_dir_labels, g, b, 0, s, root, flag, rank, m, labels, ctrl + 8);
    ROGTK_HIP_CHECK(hipGetLastError());
    uint32_t total = 0;
    ROGTK_HIP_CHECK(hipMemcpyAsync(&total, ctrl + 8, 4, hipMemcpyDeviceToHost, s));
    ROGTK_HIP_CHECK(hipStreamSynchronize(s));
    *n_clusters = (int64_t)total;
    return ROGTK_OK;
}

int directional_cluster(const DevCol& col, int L, uint32_t* cluster_id, uint64_t* root_code, int64_t* n_clusters,
                        int64_t* rounds, int64_t* longest, hipStream_t s) {
    const auto [offsets, ow, values, validity, voff, n] = col;
    *n_clusters = 0;
    *rounds = 0;
    if (longest) *longest = 0;
    if (n <= 0) return ROGTK_OK;
    ROGTK_REQUIRE(n < (1ll << 31), ROGTK_E_UNSUPPORTED, "directional: at most 2^31 - 1 rows");
    if (root_code) ROGTK_HIP_CHECK(hipMemsetAsync(root_code, 0xFF, (size_t)n * 8, s));
    int64_t codes_b = 0;  // root, labels and the scratch of directional_codes ride in the front end's codes arena
    const ExtraCodeBytes extra = [&](int64_t m, size_t* bytes) {
        if (int rc = directional_codes_temp(m, L, &codes_b)) return rc;
        *bytes = 2 * al((size_t)m * 4) + al((size_t)codes_b);
        return (int)ROGTK_OK;
    };
    SortedCodes sc;
    if (int rc = sorted_distinct_codes(col, L, true, &extra, cluster_id, &sc, s))
        return rc;
    if (longest) *longest = std::max<int64_t>(sc.max_irr_len, sc.n_reg > 0 ? L : 0);
    const int64_t m = sc.m;
    int64_t* stats = sc.spare;
    int64_t n_reg_clusters = 0;
    if (sc.n_reg > 0) {
        uint32_t* root = sc.codes_mem.take<uint32_t>(m);
        uint32_t* labels = sc.codes_mem.take<uint32_t>(m);
        void* ctemp = sc.codes_mem.take<uint8_t>(codes_b);
        if (int rc = directional_codes(sc.D, sc.C, m, L, root, labels, &n_reg_clusters, rounds, ctemp, codes_b, s))
            return rc;
        hipLaunchKernelGGL(k_dir_rows, dim3(grid_for(sc.n_reg, kBlock)), dim3(kBlock), 0, s, sc.row, sc.idx, sc.n_reg,
                           labels, root, sc.D, cluster_id, root_code);
        ROGTK_HIP_CHECK(hipGetLastError());
    }
    int64_t n_irr_clusters = 0;
    if (sc.n_irr > 0) {
        hipLaunchKernelGGL(k_dir_stats, dim3(1), dim3(1), 0, s, stats, n_reg_clusters);
        ROGTK_HIP_CHECK(hipGetLastError());
        if (int rc = irregular_cluster(offsets, ow, values, sc.irr, sc.n_irr, sc.max_irr_len, stats, cluster_id,
                                       &n_irr_clusters, s))
            return rc;
    }
    *n_clusters = n_reg_clusters + n_irr_clusters;
    ROGTK_HIP_CHECK(hipStreamSynchronize(s));  // the arenas are released behind the last kernel
    return ROGTK_OK;
}

}  // namespace rogtk
