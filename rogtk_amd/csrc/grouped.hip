// grouped.hip — UMI clustering within groups on gfx950.
//
// Every row carries a u32 key (its cell, gene, position ...). Two rows may share a cluster only
// under equal keys; within a key the rule is the ungrouped one. The key runs through the stages
// of directional.hip as the high digits of the sort key:
//
//   count   the shared front end (sorted_codes.hip) with `groups`: D[m] holds the sorted distinct
//           composites key << 2 L | code, C[m] their rows. The sort runs over 2 L +
//           bit_width(largest key) bits.
//   edges   directional_codes on the composites. A substitution touches the low 2 L bits alone
//           and a neighbour is looked up by exact value, so the graph is already the per-key
//           one, and the index order of D is (key, code): the tie order and the id order of
//           the spec. What the key changes is the search window: the edge kernel clamps it to
//           the key's own range of D, found by galloping out from the code (the default) or
//           read from a table of the key heads (k_grp_heads, a scan, k_grp_starts; kept for
//           the measurement): directional.hip, k_dir_edges<WINDOW>.
//   rows    every sorted regular row takes the label of its composite; root_code is the root's
//           composite masked down to the code. cluster_group[label] = key, written by every
//           composite of the cluster with the same value.
//   max_distance 0: no edges and no rounds, the label of a composite is its index in D.
//   irregular rows: the distinct (key, bytes) pairs after the regular clusters (irregular.hip).
#include <hipcub/hipcub.hpp>

#include <atomic>

#include "column_util.h"
#include "level2.h"

namespace rogtk {
namespace {

constexpr int kBlock = 256;
std::atomic<int> g_window{kWindowGallop};  // the faster of the two clamps by a hair, and no table (§4d)

__device__ __forceinline__ uint64_t key_of(uint64_t composite, int shift) {
    return shift < 64 ? composite >> shift : 0ull;
}

// 1 where a composite's key differs from its predecessor's (entry 0: 0): the inclusive scan is
// the rank of the key among the distinct keys
__global__ void k_grp_heads(const uint64_t* __restrict__ D, int64_t m, int shift, uint32_t* __restrict__ flag) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= m) return;
    flag[v] = v > 0 && key_of(D[v], shift) != key_of(D[v - 1], shift);
}

// gstart[rank of a key] = its first index in D; one more entry, m, closes the last range
__global__ void k_grp_starts(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ gidx, int64_t m,
                             uint32_t* __restrict__ gstart) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= m) return;
    if (v == 0 || flag[v]) gstart[gidx[v]] = (uint32_t)v;
    if (v == m - 1) gstart[gidx[v] + 1] = (uint32_t)m;
}

// every sorted regular row: the label of its composite (labels NULL: its index in D) and the
// code of its root (root NULL: its own)
__global__ void k_grp_rows(const uint32_t* __restrict__ row, const uint32_t* __restrict__ idx, int64_t n,
                           const uint32_t* __restrict__ labels, const uint32_t* __restrict__ root,
                           const uint64_t* __restrict__ D, uint64_t code_mask, uint32_t* __restrict__ cluster_id,
                           uint64_t* __restrict__ root_code) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n) return;
    const uint32_t j = idx[k], i = row[k];
    cluster_id[i] = labels ? labels[j] : j;
    if (root_code) root_code[i] = D[root ? root[j] : j] & code_mask;
}

// the key of every regular cluster; all composites of a cluster carry the same key
__global__ void k_grp_cluster_group(const uint64_t* __restrict__ D, const uint32_t* __restrict__ labels, int64_t m,
                                    int shift, uint32_t* __restrict__ cluster_group) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= m) return;
    cluster_group[labels ? labels[v] : (uint32_t)v] = (uint32_t)key_of(D[v], shift);
}

}  // namespace

int grouped_set_window(int window) {
    ROGTK_REQUIRE(window == kWindowValue || window == kWindowTable || window == kWindowGallop, ROGTK_E_INVALID,
                  "grouped window %d: 0 (value bound), 1 (table) or 2 (gallop)", window);
    g_window.store(window);
    return ROGTK_OK;
}

int grouped_cluster(const DevCol& col, int L, const uint32_t* groups, int max_distance, uint32_t* cluster_id,
                    uint64_t* root_code, uint32_t* cluster_group, int64_t* n_clusters, int64_t* rounds,
                    int64_t* longest, hipStream_t s) {
    const auto [offsets, ow, values, validity, voff, n] = col;
    *n_clusters = 0;
    *rounds = 0;
    if (longest) *longest = 0;
    if (n <= 0) return ROGTK_OK;
    ROGTK_REQUIRE(n < (1ll << 31), ROGTK_E_UNSUPPORTED, "grouped: at most 2^31 - 1 rows");
    ROGTK_REQUIRE(groups, ROGTK_E_INVALID, "grouped: NULL groups");
    ROGTK_REQUIRE(max_distance == 0 || max_distance == 1, ROGTK_E_UNSUPPORTED,
                  "max_distance %d: only 0 and 1 are supported", max_distance);
    const bool edges = max_distance == 1;
    const int window = g_window.load();
    const bool table = edges && window == kWindowTable;
    if (root_code) ROGTK_HIP_CHECK(hipMemsetAsync(root_code, 0xFF, (size_t)n * 8, s));
    int64_t codes_b = 0;
    size_t scan_b = 0;
    const ExtraCodeBytes extra = [&](int64_t m, size_t* bytes) -> int {
        *bytes = 0;
        if (!edges) return (int)ROGTK_OK;
        if (int rc = directional_codes_temp(m, L, &codes_b)) return rc;
        *bytes = 2 * al((size_t)m * 4) + al((size_t)codes_b);
        if (table) {
            ROGTK_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, scan_b, (const uint32_t*)nullptr,
                                                             (uint32_t*)nullptr, (int)m, s));
            *bytes += 2 * al((size_t)m * 4) + al((size_t)(m + 1) * 4) + al(scan_b);
        }
        return (int)ROGTK_OK;
    };
    SortedCodes sc;
    if (int rc = sorted_distinct_codes(col, L, true, &extra, cluster_id, &sc, s,
                                       groups))
        return rc;
    if (longest) *longest = std::max<int64_t>(sc.max_irr_len, sc.n_reg > 0 ? L : 0);
    const int64_t m = sc.m;
    const int shift = 2 * L;  // n_reg > 0 only for L 1..32
    int64_t n_reg_clusters = 0;
    if (sc.n_reg > 0) {
        const dim3 g(grid_for(m, kBlock)), b(kBlock);
        const uint64_t code_mask = shift < 64 ? (1ull << shift) - 1ull : ~0ull;
        uint32_t *root = nullptr, *labels = nullptr;
        if (edges) {
            root = sc.codes_mem.take<uint32_t>(m);
            labels = sc.codes_mem.take<uint32_t>(m);
            void* ctemp = sc.codes_mem.take<uint8_t>(codes_b);
            DirGroups grp{shift, window, nullptr, nullptr};
            if (table) {
                uint32_t* gflag = sc.codes_mem.take<uint32_t>(m);
                uint32_t* gidx = sc.codes_mem.take<uint32_t>(m);
                uint32_t* gstart = sc.codes_mem.take<uint32_t>(m + 1);
                void* stmp = sc.codes_mem.take<uint8_t>((int64_t)scan_b);
                hipLaunchKernelGGL(k_grp_heads, g, b, 0, s, sc.D, m, shift, gflag);
                size_t sb = scan_b;
                ROGTK_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(stmp, sb, gflag, gidx, (int)m, s));
                hipLaunchKernelGGL(k_grp_starts, g, b, 0, s, gflag, gidx, m, gstart);
                ROGTK_HIP_CHECK(hipGetLastError());
                grp.gidx = gidx;
                grp.gstart = gstart;
            }
            if (int rc = directional_codes(sc.D, sc.C, m, L, root, labels, &n_reg_clusters, rounds, ctemp, codes_b, s,
                                           &grp))
                return rc;
        } else {
            n_reg_clusters = m;
        }
        hipLaunchKernelGGL(k_grp_rows, dim3(grid_for(sc.n_reg, kBlock)), b, 0, s, sc.row, sc.idx, sc.n_reg, labels,
                           root, sc.D, code_mask, cluster_id, root_code);
        if (cluster_group) hipLaunchKernelGGL(k_grp_cluster_group, g, b, 0, s, sc.D, labels, m, shift, cluster_group);
        ROGTK_HIP_CHECK(hipGetLastError());
    }
    int64_t n_irr_clusters = 0;
    if (sc.n_irr > 0)
        if (int rc = irregular_cluster_grouped(offsets, ow, values, sc.irr, sc.n_irr, sc.max_irr_len, groups,
                                               sc.max_irr_group, (uint32_t)n_reg_clusters, cluster_id, cluster_group,
                                               &n_irr_clusters, s))
            return rc;
    *n_clusters = n_reg_clusters + n_irr_clusters;
    ROGTK_HIP_CHECK(hipStreamSynchronize(s));  // the arenas are released behind the last kernel
    return ROGTK_OK;
}

}  // namespace rogtk
