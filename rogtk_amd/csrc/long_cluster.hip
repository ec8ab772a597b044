// long_cluster.hip — H3 for UMIs of 17..32 bases, where the 4^L presence
// bitmap of the packed engine (cluster_kernels.hip, L <= 16) stops being affordable.
//
// Same specification and ids as the packed engine and the oracle
// (oracle/rogtk_oracle.cpp: oracle_umi_cluster packs L <= 32):
//   * regular rows (valid, byte length L, pure ACGT) -> 2-bit codes in a u64;
//   * max_distance 0: one cluster per distinct code; 1: connected components of the
//     distinct codes under Hamming distance 1;
//   * ids dense in order of each cluster's smallest code; irregular rows grouped by
//     exact bytes after them (irregular.hip); null rows 0xFFFFFFFF.
//
// Sort-based, no code-space tables:
//   1. the shared front end (sorted_codes.hip): the regular rows sorted by code, the sorted
//      distinct codes D and each sorted row's index into D;
//   2. one record (code with digit p zeroed, p, code) per distinct code and position,
//      sorted by masked code then stably by p: equal (p, key) runs are the codes that
//      differ only at p (a clique); consecutive members give edges (dist_cluster.hip);
//   3. the shared connected-components back end (cc_labels, dist_cluster.hip): one dense
//      label per distinct code, in order of each component's smallest code;
//   4. labels -> rows.
#include <cstdlib>

#include "column_util.h"
#include "level2.h"

namespace rogtk {
namespace {

constexpr int kB = 256;
// (code, position) records per edge-finding batch; ROGTK_LONG_REC_BATCH overrides (read
// per call: tests lower it to cover the batching)
inline int64_t rec_batch() {
    const char* e = getenv("ROGTK_LONG_REC_BATCH");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (int64_t)v : (int64_t)1 << 28;
}

// labels NULL (max_distance 0): a row's id is its code's index among the distinct codes
__global__ __launch_bounds__(kB) void k_assign_long(const uint32_t* __restrict__ row, const uint32_t* __restrict__ idx,
                                                    int64_t n, const uint32_t* __restrict__ labels,
                                                    uint32_t* __restrict__ cid) {
    const int64_t k = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (k >= n) return;
    const uint32_t d = idx[k];
    cid[row[k]] = labels ? labels[d] : d;
}

__global__ void k_put_count(int64_t* stats, int64_t v) { stats[1] = v; }

// Hamming-1 edges among the distinct codes D[nd] into E (room for nd * L): one record
// (code with digit p zeroed, p, code) per distinct code and position, grouped by (p, masked
// code) with two sorts (dist_cluster.hip, the steps of the sharded engine at world 1)
// instead of one sort per position: 1.7x faster at L = 20 (10M reads). Positions go in
// batches of <= rec_batch() records (nd * L may pass 2^31, the sorts' limit; the batch also
// bounds the 20 B/record scratch).
int clique_edges(const uint64_t* D, int64_t nd, int L, uint2* E, int64_t* n_edges, hipStream_t s) {
    ROGTK_REQUIRE(nd < (1ll << 31), ROGTK_E_UNSUPPORTED, "long_cluster: 2^31 distinct UMIs");
    const int64_t per = std::max<int64_t>(1, std::min<int64_t>(L, rec_batch() / std::max<int64_t>(nd, 1)));
    const int64_t nrec_max = nd * per;
    Arena R;
    if (int rc = R.get(2 * al((size_t)nrec_max * 8) + al((size_t)nrec_max * 4), s)) return rc;
    uint64_t* rmk = R.take<uint64_t>(nrec_max);
    uint32_t* rpos = R.take<uint32_t>(nrec_max);
    uint64_t* rcode = R.take<uint64_t>(nrec_max);
    int64_t ne = 0;
    for (int p0 = 0; p0 < L; p0 += (int)per) {
        const int np = (int)std::min<int64_t>(per, L - p0);
        if (int rc = masked_records_range(D, nd, p0, np, rmk, rpos, rcode, s)) return rc;
        int64_t got = 0;
        if (int rc = rogtk_clique_edges(rmk, rpos, rcode, nd * np, L, D, nd, (uint32_t*)(E + ne), &got, s)) return rc;
        ne += got;
    }
    *n_edges = ne;
    return ROGTK_OK;
}

}  // namespace

int long_cluster(const DevCol& col, int L, int max_distance, int64_t max_len, uint32_t* cid, int64_t* n_clusters,
                 hipStream_t s) {
    const auto [offsets, ow, values, validity, voff, n] = col;
    ROGTK_REQUIRE(L > kMaxPackedLen && L <= 32, ROGTK_E_UNSUPPORTED, "long_cluster: umi_len %d outside 17..32", L);
    ROGTK_REQUIRE(n < (1ll << 31), ROGTK_E_UNSUPPORTED, "long_cluster: more than 2^31 rows");
    if (n_clusters) *n_clusters = 0;
    if (n <= 0) return ROGTK_OK;
    ProfScope prof(K_UNION, s);
    // max_distance 1: the labels and the edges ride in the front end's codes arena
    const ExtraCodeBytes extra = [&](int64_t m, size_t* bytes) {
        *bytes = max_distance == 1 ? al((size_t)m * 4) + al((size_t)m * L * 8) : 0;
        return (int)ROGTK_OK;
    };
    SortedCodes sc;
    if (int rc = sorted_distinct_codes(col, L, false, &extra, cid, &sc, s))
        return rc;
    const int64_t nd = sc.m;  // distinct regular codes
    int64_t* stats = sc.spare;
    uint32_t* labels = nullptr;  // one per distinct code (max_distance 1)
    int64_t n_reg_clusters = nd;
    if (sc.n_reg > 0) {
        if (max_distance == 1) {
            labels = sc.codes_mem.take<uint32_t>(nd);
            uint2* E = sc.codes_mem.take<uint2>(nd * (int64_t)L);
            int64_t ne = 0;
            if (int rc = clique_edges(sc.D, nd, L, E, &ne, s)) return rc;
            if (int rc = cc_labels(nd, (const uint32_t*)E, ne, labels, &n_reg_clusters, s)) return rc;
        }
        hipLaunchKernelGGL(k_assign_long, dim3(grid_for(sc.n_reg, kB)), dim3(kB), 0, s, sc.row, sc.idx, sc.n_reg,
                           labels, cid);
        ROGTK_HIP_CHECK(hipGetLastError());
    }
    int64_t total = n_reg_clusters;
    if (sc.n_irr > 0 && max_distance == 1) {
        // Hamming-1 edges of the irregular rows, merged with the regular clusters
        // (irregular.hip); the lookup binary-searches the sorted distinct codes
        CodeLookup lk = [&](const uint64_t* q, int64_t nq, uint32_t* lab, hipStream_t st) {
            return sorted_code_lookup(sc.D, nd, labels, q, nq, lab, st);
        };
        if (int rc = irregular_merge(offsets, ow, values, sc.irr, sc.n_irr, max_len, L, n_reg_clusters,
                                     nd > 0 ? &lk : nullptr, cid, n, cid, &total, s))
            return rc;
    } else if (sc.n_irr > 0) {
        int64_t n_irr_clusters = 0;
        hipLaunchKernelGGL(k_put_count, dim3(1), dim3(1), 0, s, stats, n_reg_clusters);
        if (int rc = irregular_cluster(offsets, ow, values, sc.irr, sc.n_irr, max_len, stats, cid, &n_irr_clusters, s))
            return rc;
        total += n_irr_clusters;
    }
    ROGTK_HIP_CHECK(hipStreamSynchronize(s));
    if (n_clusters) *n_clusters = total;
    return ROGTK_OK;
}

}  // namespace rogtk
