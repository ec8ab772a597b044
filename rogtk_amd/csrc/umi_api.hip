// umi_api.hip — the UMI cluster / correct family of the C ABI (include/rogtk_hip.h; DESIGN.md
// §4g): rogtk_umi_{cluster,correct}[_directional|_grouped]_{host,dev}, the cluster summary
// entries, and the directional / grouped code-level entries.
//
// All twelve ids entries ask one question, "ids for this device column under this rule", and
// cluster_ids() is the one place that answers it: it alone chooses between grouped_cluster,
// directional_cluster and stage -> cluster_staged. An entry is check -> (upload) ->
// cluster_ids -> (summary and gather, or download); check_cluster_call holds the argument
// rules of all twelve and runs before the first device access (host_ctx()).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "level2.h"

using namespace rogtk;

namespace {

thread_local int64_t t_directional_rounds = 0;  // rogtk_directional_last_rounds

// method: 0 cluster (the H3 components), 1 directional. groups: one u32 key per
// row, NULL for an ungrouped call; on the device where cluster_ids sees it.
struct ClusterRule {
    int method;
    int max_distance;
    const uint32_t* groups;
    // without edges the directional rule is the exact grouping of the cluster method: one
    // implementation
    bool relaxes() const { return method == 1 && max_distance == 1; }
};

// ids / root_code / cluster_group: the caller's device arrays (the last two nullable).
// want_max_len: the caller goes on to the summary, whose sort max_len bounds. n_clusters and
// max_len (the longest row) are results; max_len may stay 0 when it was not wanted.
struct ClusterIds {
    uint32_t* ids;
    uint64_t* root_code;
    uint32_t* cluster_group;
    bool want_max_len;
    int64_t n_clusters;
    int64_t max_len;
};

ClusterRule grouped_rule(int method, int max_distance, const uint32_t* groups) {
    static const uint32_t no_rows = 0;  // an empty column still takes the grouped path
    return ClusterRule{method, max_distance, groups ? groups : &no_rows};
}

// what check_cluster_call looks at besides the rule
enum : unsigned {
    kRowLimit = 1,   // n < 2^31 (ROGTK_E_UNSUPPORTED); the two plain cluster entries have no limit
    kGrouped = 2,    // the method rules of the grouped entries
    kDeviceCol = 4,  // a device column: umi_len is given, not resolved from the first row
    kNullArg = 8,    // the entry found one of its required buffers NULL (with n > 0)
};
unsigned null_arg(bool all_given) { return all_given ? 0u : kNullArg; }

// The argument rules of the twelve ids entries (include/rogtk_hip.h), before any device work.
int check_cluster_call(const char* name, int64_t n, int umi_len, const ClusterRule& rule, unsigned flags) {
    if (flags & kRowLimit)
        if (int rc = check_rows_and_clusters(name, n, 0)) return rc;
    if (flags & kGrouped)
        ROGTK_REQUIRE(rule.method == 0 || rule.method == 1, ROGTK_E_INVALID,
                      "%s: method %d is neither 0 (cluster) nor 1 (directional)", name, rule.method);
    ROGTK_REQUIRE(rule.max_distance == 0 || rule.max_distance == 1, ROGTK_E_UNSUPPORTED,
                  "max_distance %d: only 0 and 1 are supported", rule.max_distance);
    if (flags & kGrouped)
        ROGTK_REQUIRE(rule.method == 1 || rule.max_distance == 0, ROGTK_E_UNSUPPORTED,
                      "%s: method=\"cluster\" with max_distance 1 is not supported within groups (irregular strings "
                      "bridge clusters under the transitive rule); use method=\"directional\"",
                      name);
    ROGTK_REQUIRE(n >= 0 && !(flags & kNullArg), ROGTK_E_INVALID, "%s: NULL argument (or n < 0)", name);
    ROGTK_REQUIRE(!(flags & kDeviceCol) || umi_len >= 1, ROGTK_E_INVALID, "%s: umi_len must be >= 1", name);
    return ROGTK_OK;
}

// what an ids entry leaves for a column without rows
void begin_ids(const ClusterRule& rule, int64_t* n_clusters) {
    if (n_clusters) *n_clusters = 0;
    if (rule.groups || rule.relaxes()) t_directional_rounds = 0;
}

// H3 over a column already staged into c->codes / regbits / irr (n_irr irregular rows):
// regular rows through the cluster engine, then the irregular rows (exact bytes, or for
// max_distance 1 their Hamming-1 edges merged with the regular clusters, irregular.hip);
// ids into did (device), on stream s.
int cluster_staged(HostCtx* c, const DevCol& col, int L, int64_t n_irr, int64_t max_len, int max_distance,
                   uint32_t* did, int64_t* n_clusters, hipStream_t s) {
    if (L > kMaxPackedLen && L <= 32)  // long UMIs: sort-based engine (regular + irregular rows)
        return long_cluster(col, L, max_distance, max_len, did, n_clusters, s);
    const int64_t n = col.n;
    int64_t n_reg_clusters = 0;
    const int64_t* stats_dev = nullptr;
    if (L >= 1 && L <= kMaxPackedLen) {
        const int64_t space = (int64_t)1 << std::min(2 * L, 40);
        const int64_t maxd = std::max<int64_t>(1, std::min<int64_t>(space, n));
        ClusterLayout cl;
        if (int rc = cluster_layout(L, maxd, &cl)) return rc;
        if (c->ws_L != L || c->ws_maxd < cl.max_distinct) {
            if (int rc = c->ws.ensure((size_t)cl.total)) return rc;
            if (int rc = rogtk_cluster_init(c->ws.p, L, cl.max_distinct, s)) return rc;
            c->ws_L = L;
            c->ws_maxd = cl.max_distinct;
        }
        ClusterLayout use;
        cluster_layout(L, c->ws_maxd, &use);
        if (int rc = c->bitmap.ensure((size_t)use.words * 8)) return rc;
        int rc = rogtk_cluster_mark(c->codes.as<uint32_t>(), c->regbits.as<uint64_t>(), n, L, c->ws.p,
                                    use.max_distinct, s);
        if (!rc) rc = rogtk_cluster_local_bitmap(c->ws.p, L, use.max_distinct, c->bitmap.as<uint64_t>(), s);
        if (!rc) rc = rogtk_cluster_resolve(c->ws.p, L, use.max_distinct, c->bitmap.as<uint64_t>(), 1,
                                            max_distance, s);
        if (!rc) rc = rogtk_cluster_assign(c->ws.p, L, use.max_distinct, c->codes.as<uint32_t>(),
                                           c->regbits.as<uint64_t>(), n, did, s);
        if (rc) {
            c->ws_L = -1;  // presence may be dirty: re-initialise on the next call
            return rc;
        }
        int64_t st[4];
        if (int rc2 = rogtk_cluster_stats(c->ws.p, L, use.max_distinct, st, s)) return rc2;
        ROGTK_REQUIRE(st[2] == 0, ROGTK_E_OVERFLOW, "cluster: distinct UMIs exceeded max_distinct");
        n_reg_clusters = st[1];
        stats_dev = (const int64_t*)((uint8_t*)c->ws.p + use.off_stats);
    } else {
        ROGTK_HIP_CHECK(hipMemsetAsync(did, 0xFF, (size_t)n * 4, s));
    }
    int64_t total = n_reg_clusters;
    if (n_irr > 0 && max_distance == 1) {
        // Hamming-1 edges of the irregular rows (to each other and to regular codes)
        const bool packable = L >= 1 && L <= kMaxPackedLen;
        ClusterLayout use{};
        if (packable) cluster_layout(L, c->ws_maxd, &use);
        const uint8_t* ws = (const uint8_t*)c->ws.p;
        CodeLookup lk = [&](const uint64_t* q, int64_t nq, uint32_t* lab, hipStream_t st) {
            return launch_cluster_lookup(use, ws, q, nq, lab, st);
        };
        int rc = irregular_merge(col.offsets, col.ow, col.values, c->irr.as<int64_t>(), n_irr, max_len, L,
                                 n_reg_clusters, packable ? &lk : nullptr, did, n, did, &total, s);
        if (rc) return rc;
    } else if (n_irr > 0) {
        int64_t n_irr_clusters = 0;
        int rc = irregular_cluster(col.offsets, col.ow, col.values, c->irr.as<int64_t>(), n_irr, max_len, stats_dev,
                                   did, &n_irr_clusters, s);
        if (rc) return rc;
        total += n_irr_clusters;
    }
    if (n_clusters) *n_clusters = total;
    return ROGTK_OK;
}

// Ids of a device column of n >= 1 rows under a rule, on stream s (synchronised on return).
// out->max_len: the directional and grouped engines report the longest non-null row, the
// cluster method the longest row of any validity (k_max_len). The value only bounds a sort
// width, and each engine keeps its own.
int cluster_ids(HostCtx* c, const DevCol& col, int L, const ClusterRule& rule, ClusterIds* out, hipStream_t s) {
    if (rule.groups)
        return grouped_cluster(col, L, rule.groups, rule.max_distance, out->ids, out->root_code, out->cluster_group,
                               &out->n_clusters, &t_directional_rounds, &out->max_len, s);
    if (rule.relaxes())
        return directional_cluster(col, L, out->ids, out->root_code, &out->n_clusters, &t_directional_rounds,
                                   &out->max_len, s);
    int64_t hv[2] = {0, 0};  // the irregular rows, the longest row
    if (out->want_max_len || (L > kMaxPackedLen && L <= 32)) {  // both words in one read-back and one sync
        if (int rc = stage_uploaded(c, col, L, nullptr, s)) return rc;
        unsigned long long* cnt = c->nirr.as<unsigned long long>();
        if (int rc = launch_max_len(col.offsets, col.ow, col.n, cnt + 1, s)) return rc;
        ROGTK_HIP_CHECK(hipMemcpyAsync(hv, cnt, 16, hipMemcpyDeviceToHost, s));
        ROGTK_HIP_CHECK(hipStreamSynchronize(s));
    } else {  // only the irregular rows' sort needs the longest row: a regular column skips k_max_len
        if (int rc = stage_uploaded(c, col, L, &hv[0], s)) return rc;
        if (hv[0] > 0)
            if (int rc = column_max_len(col.offsets, col.ow, col.n, c->nirr.as<unsigned long long>() + 1, s, &hv[1]))
                return rc;
    }
    out->max_len = hv[1];
    return cluster_staged(c, col, L, hv[0], hv[1], rule.max_distance, out->ids, &out->n_clusters, s);
}

// the three per-cluster tables of a column with its ids into c->out[1..3] (n_reads, n_distinct,
// the row that holds the representative)
int summary_tables(HostCtx* c, const DevCol& col, int L, const uint32_t* ids, int64_t nclu, int64_t max_len,
                   hipStream_t s) {
    const int64_t nc1 = std::max<int64_t>(nclu, 1);
    if (c->out[1].ensure((size_t)nc1 * 4) || c->out[2].ensure((size_t)nc1 * 4) || c->out[3].ensure((size_t)nc1 * 8))
        return ROGTK_E_HIP;
    return cluster_summary_general(col, L, ids, nclu, max_len, c->out[1].as<uint32_t>(), c->out[2].as<uint32_t>(),
                                   c->out[3].as<int64_t>(), s);
}

// The summary of a column on the context's device buffers (ids in did): counts to the host
// results, representatives measured, filled and copied into `reps`.
int summary_to_host(HostCtx* c, const DevCol& col, int L, const uint32_t* did, int64_t nclu, int64_t max_len,
                    rogtk_str_result* reps, rogtk_u32_result* n_reads, rogtk_u32_result* n_distinct) {
    hipStream_t s = c->stream;
    int64_t tb = 0;
    if (int rc = representatives_temp(nclu, &tb)) return rc;
    if (c->out[4].ensure((size_t)(nclu + 1) * 8) || c->out[5].ensure((size_t)tb)) return ROGTK_E_HIP;
    if (int rc = summary_tables(c, col, L, did, nclu, max_len, s)) return rc;
    const int64_t* rep_row = c->out[3].as<int64_t>();
    if (int rc = representatives_measure(col, rep_row, nclu, c->out[4].as<int64_t>(), c->out[5].p, tb, s)) return rc;
    for (rogtk_u32_result* r : {n_reads, n_distinct}) {
        r->n = nclu;
        r->data = (uint32_t*)calloc((size_t)std::max<int64_t>(nclu, 1), 4);
        ROGTK_REQUIRE(r->data, ROGTK_E_INVALID, "out of host memory");
    }
    if (nclu > 0) {
        if (int rc = c->d2h(n_reads->data, c->out[1].p, (size_t)nclu * 4)) return rc;
        if (int rc = c->d2h(n_distinct->data, c->out[2].p, (size_t)nclu * 4)) return rc;
    }
    if (int rc = str_result_begin(c, nclu, c->out[4].as<int64_t>(), nullptr, nullptr, reps)) return rc;
    return str_result_finish(
        c, c->out[6],
        [&](uint8_t* d) {
            return representatives_fill(col.offsets, col.ow, col.values, rep_row, nclu, c->out[4].as<int64_t>(), d, s);
        },
        reps);
}

int check_correct_outputs(const rogtk_str_col* col, rogtk_str_result* reps, rogtk_u32_result* n_reads,
                          rogtk_u32_result* n_distinct) {
    ROGTK_REQUIRE(col, ROGTK_E_INVALID, "NULL column");
    ROGTK_REQUIRE(reps && n_reads && n_distinct, ROGTK_E_INVALID,
                  "NULL output (representatives, n_reads and n_distinct are required)");
    *reps = rogtk_str_result{};
    u32_result_reset(n_reads);
    u32_result_reset(n_distinct);
    return ROGTK_OK;
}

// the keys of a host column on the device (c->grp[0]) and room for the clusters' keys (c->grp[1])
int upload_groups(HostCtx* c, const uint32_t* groups, int64_t n) {
    const size_t b = (size_t)std::max<int64_t>(n, 1) * 4;
    if (int rc = c->grp[0].ensure(b)) return rc;
    if (int rc = c->grp[1].ensure(b)) return rc;
    return c->h2d(c->grp[0].p, groups, (size_t)n * 4);
}

int groups_to_host(HostCtx* c, int64_t nclu, rogtk_u32_result* cluster_group) {
    if (!cluster_group) return ROGTK_OK;
    cluster_group->n = nclu;
    cluster_group->data = (uint32_t*)calloc((size_t)std::max<int64_t>(nclu, 1), 4);
    ROGTK_REQUIRE(cluster_group->data, ROGTK_E_INVALID, "out of host memory");
    return c->d2h(cluster_group->data, c->grp[1].p, (size_t)nclu * 4);
}

// The host entries' way to cluster_ids: the column (and rule.groups, here the host's keys) onto
// the context's buffers, ids into c->out[0] (the clusters' keys into c->grp[1]) and on to
// cluster_id. A column without rows leaves *ids empty and *col without buffers.
int host_ids(HostCtx* c, const HostCol& h, int L, ClusterRule rule, bool want_max_len, uint32_t* cluster_id,
             ClusterIds* ids, DevCol* col) {
    const int64_t n = h.n;
    if (int rc = c->out[0].ensure((size_t)std::max<int64_t>(n, 4) * 4)) return rc;
    *ids = ClusterIds{c->out[0].as<uint32_t>(), nullptr, nullptr, want_max_len, 0, 0};
    *col = DevCol(nullptr, h.ow, nullptr, nullptr, h.voff, 0);
    if (n == 0) return ROGTK_OK;
    if (int rc = upload_col(c, 0, h, col)) return rc;
    if (rule.groups) {
        if (int rc = upload_groups(c, rule.groups, n)) return rc;
        rule.groups = c->grp[0].as<uint32_t>();
        ids->cluster_group = c->grp[1].as<uint32_t>();
    }
    if (int rc = cluster_ids(c, *col, L, rule, ids, c->stream)) return rc;
    return c->d2h(cluster_id, ids->ids, (size_t)n * 4);
}

// the three host cluster entries after their own NULL checks (in flags)
int cluster_host(const char* name, const HostCol& h, int umi_len, const ClusterRule& rule, unsigned flags,
                 uint32_t* cluster_id, int64_t* n_clusters, int* resolved_umi_len, rogtk_u32_result* cluster_group) {
    u32_result_reset(cluster_group);
    if (int rc = check_host_col(h)) return rc;
    if (int rc = check_cluster_call(name, h.n, umi_len, rule, flags)) return rc;
    const int L = umi_len > 0 ? umi_len : h.first_len();
    if (resolved_umi_len) *resolved_umi_len = L;
    begin_ids(rule, n_clusters);
    if (h.n == 0) return ROGTK_OK;
    HostCtx* c;
    if (int rc = host_ctx(&c)) return rc;
    ClusterIds ids;
    DevCol dcol;
    if (int rc = host_ids(c, h, L, rule, false, cluster_id, &ids, &dcol)) return rc;
    if (n_clusters) *n_clusters = ids.n_clusters;
    const int rc = groups_to_host(c, ids.n_clusters, cluster_group);
    if (rc) rogtk_u32_result_free(cluster_group);
    return rc;
}

// the three host correct entries: ids, their summary, and every row's bytes from its cluster's
// representative
int correct_host(const char* name, const rogtk_str_col* col, int umi_len, const ClusterRule& rule, unsigned flags,
                 uint32_t* cluster_id, rogtk_str_result* corrected, rogtk_str_result* representatives,
                 rogtk_u32_result* n_reads, rogtk_u32_result* n_distinct, rogtk_u32_result* cluster_group,
                 int64_t* n_clusters, int* resolved_umi_len) {
    u32_result_reset(cluster_group);
    if (int rc = check_correct_outputs(col, representatives, n_reads, n_distinct)) return rc;
    ROGTK_REQUIRE(corrected, ROGTK_E_INVALID, "NULL output (corrected is required)");
    *corrected = rogtk_str_result{};
    const HostCol h(*col);
    if (int rc = check_host_col(h)) return rc;
    const int64_t n = h.n;
    if (int rc = check_cluster_call(name, n, umi_len, rule, flags | kRowLimit | null_arg(cluster_id || n == 0)))
        return rc;
    const int L = umi_len > 0 ? umi_len : h.first_len();
    if (resolved_umi_len) *resolved_umi_len = L;
    if (n_clusters) *n_clusters = 0;
    if (rule.groups) t_directional_rounds = 0;  // ungrouped: an empty column leaves the last call's rounds
    HostCtx* c;
    if (int rc = host_ctx(&c)) return rc;
    auto run = [&]() -> int {
        ClusterIds ids;
        DevCol dcol;
        if (int rc = host_ids(c, h, L, rule, true, cluster_id, &ids, &dcol)) return rc;
        const int64_t nclu = ids.n_clusters;
        if (n_clusters) *n_clusters = nclu;
        if (rule.groups)
            if (int rc = groups_to_host(c, nclu, cluster_group)) return rc;
        if (int rc = summary_to_host(c, dcol, L, ids.ids, nclu, ids.max_len, representatives, n_reads, n_distinct))
            return rc;
        // corrected: the input's offsets and nulls, every row's bytes from its representative
        if (int rc = str_result_begin(c, n, nullptr, nullptr, &h, corrected)) return rc;
        return str_result_finish(
            c, c->out[6],
            [&](uint8_t* d) -> int {
                ROGTK_HIP_CHECK(hipMemsetAsync(d, 0, (size_t)h.off(n), c->stream));
                return corrected_fill(dcol, ids.ids, nclu, c->out[3].as<int64_t>(), d, c->stream);
            },
            corrected);
    };
    const int rc = run();
    if (rc) {
        rogtk_str_result_free(corrected);
        rogtk_str_result_free(representatives);
        rogtk_u32_result_free(n_reads);
        rogtk_u32_result_free(n_distinct);
        rogtk_u32_result_free(cluster_group);
    }
    return rc;
}

// the six device entries after their checks: ids on the caller's stream, and for a correct entry
// (corrected_values given) the summary on the context's buffers and the gather
int ids_dev(const DevCol& col, int L, const ClusterRule& rule, ClusterIds ids, int64_t* n_clusters,
            uint8_t* corrected_values, hipStream_t s) {
    begin_ids(rule, n_clusters);
    if (col.n == 0) return ROGTK_OK;
    HostCtx* c;
    if (int rc = host_ctx(&c)) return rc;
    ids.want_max_len = true;  // also the ids-only device entry keeps its one read-back and one sync
    if (int rc = cluster_ids(c, col, L, rule, &ids, s)) return rc;
    if (n_clusters) *n_clusters = ids.n_clusters;
    if (!corrected_values) return ROGTK_OK;
    if (int rc = summary_tables(c, col, L, ids.ids, ids.n_clusters, ids.max_len, s)) return rc;
    return corrected_fill(col, ids.ids, ids.n_clusters, c->out[3].as<int64_t>(), corrected_values, s);
}

}  // namespace

extern "C" {

// ------------------------------------------------------------ method="cluster"
int rogtk_umi_cluster_host(const void* offsets, int offset_width, const uint8_t* values, int64_t values_len,
                           const uint8_t* validity, int64_t validity_offset, int64_t n, int umi_len, int max_distance,
                           uint32_t* cluster_id, int64_t* n_clusters, int* resolved_umi_len) {
    return cluster_host("umi_cluster", HostCol(offsets, offset_width, values, values_len, validity, validity_offset, n),
                        umi_len, ClusterRule{0, max_distance, nullptr}, null_arg(cluster_id || n == 0), cluster_id,
                        n_clusters, resolved_umi_len, nullptr);
}

int rogtk_umi_cluster_dev(const int64_t* offsets, const uint8_t* values, const uint8_t* validity, int64_t n,
                          int umi_len, int max_distance, uint32_t* cluster_id, int64_t* n_clusters, void* stream) {
    const ClusterRule rule{0, max_distance, nullptr};
    if (int rc = check_cluster_call("umi_cluster_dev", n, umi_len, rule,
                                    kDeviceCol | null_arg(n == 0 || (offsets && values && cluster_id))))
        return rc;
    return ids_dev(DevCol(offsets, values, validity, n), umi_len, rule, ClusterIds{cluster_id}, n_clusters, nullptr,
                   as_stream(stream));
}

int rogtk_umi_correct_host(const rogtk_str_col* col, int umi_len, int max_distance, uint32_t* cluster_id,
                           rogtk_str_result* corrected, rogtk_str_result* representatives, rogtk_u32_result* n_reads,
                           rogtk_u32_result* n_distinct, int64_t* n_clusters, int* resolved_umi_len) {
    return correct_host("umi_correct", col, umi_len, ClusterRule{0, max_distance, nullptr}, 0, cluster_id, corrected,
                        representatives, n_reads, n_distinct, nullptr, n_clusters, resolved_umi_len);
}

int rogtk_umi_correct_dev(const int64_t* offsets, const uint8_t* values, const uint8_t* validity, int64_t n,
                          int umi_len, int max_distance, uint32_t* cluster_id, int64_t* n_clusters,
                          uint8_t* corrected_values, void* stream) {
    const ClusterRule rule{0, max_distance, nullptr};
    if (int rc = check_cluster_call("umi_correct_dev", n, umi_len, rule,
                                    kRowLimit | kDeviceCol |
                                        null_arg(n == 0 || (offsets && values && cluster_id && corrected_values))))
        return rc;
    return ids_dev(DevCol(offsets, values, validity, n), umi_len, rule, ClusterIds{cluster_id}, n_clusters,
                   corrected_values, as_stream(stream));
}

// ------------------------------------------------------------ the cluster summary (correct.hip)
int rogtk_cluster_summary_set_method(int method) { return cluster_summary_set_method(method); }

int rogtk_cluster_summary_temp_bytes(int64_t n, int umi_len, int64_t n_clusters, int64_t* bytes) {
    ROGTK_REQUIRE(bytes, ROGTK_E_INVALID, "cluster_summary_temp_bytes: NULL bytes");
    ROGTK_REQUIRE(umi_len >= 1 && umi_len <= kMaxPackedLen, ROGTK_E_UNSUPPORTED,
                  "packed cluster summary: umi_len %d outside 1..%d", umi_len, kMaxPackedLen);
    if (int rc = check_rows_and_clusters("packed cluster summary", n, n_clusters)) return rc;
    return cluster_summary_packed_temp(n, umi_len, n_clusters, bytes);
}

int rogtk_cluster_summary_packed(const uint32_t* codes, const uint64_t* regular_bits, int64_t n, int umi_len,
                                 const uint32_t* cluster_id, int64_t n_clusters, uint32_t* rep_code, uint32_t* n_reads,
                                 uint32_t* n_distinct, void* temp, int64_t temp_bytes, void* stream) {
    ROGTK_REQUIRE(umi_len >= 1 && umi_len <= kMaxPackedLen, ROGTK_E_UNSUPPORTED,
                  "packed cluster summary: umi_len %d outside 1..%d", umi_len, kMaxPackedLen);
    if (int rc = check_rows_and_clusters("packed cluster summary", n, n_clusters)) return rc;
    ROGTK_REQUIRE(n == 0 || (codes && cluster_id), ROGTK_E_INVALID, "packed cluster summary: NULL codes / cluster_id");
    ROGTK_REQUIRE(n_clusters == 0 || (rep_code && n_reads && n_distinct), ROGTK_E_INVALID,
                  "packed cluster summary: NULL output table");
    ROGTK_REQUIRE(temp, ROGTK_E_INVALID, "packed cluster summary: NULL temp");
    return launch_cluster_summary_packed(codes, regular_bits, n, umi_len, cluster_id, n_clusters, rep_code, n_reads,
                                         n_distinct, temp, temp_bytes, as_stream(stream));
}

int rogtk_cluster_correct_packed(const uint32_t* cluster_id, const uint64_t* regular_bits, int64_t n,
                                 const uint32_t* rep_code, int64_t n_clusters, uint32_t* corrected_codes,
                                 void* stream) {
    ROGTK_REQUIRE(n >= 0 && n_clusters >= 0, ROGTK_E_INVALID, "packed correct: negative size");
    ROGTK_REQUIRE(n == 0 || (cluster_id && corrected_codes && (rep_code || n_clusters == 0)), ROGTK_E_INVALID,
                  "packed correct: NULL argument");
    return launch_cluster_correct_packed(cluster_id, regular_bits, n, rep_code, n_clusters, corrected_codes,
                                         as_stream(stream));
}

int rogtk_cluster_summary_host(const rogtk_str_col* col, int umi_len, const uint32_t* cluster_id, int64_t n_clusters,
                               rogtk_str_result* representatives, rogtk_u32_result* n_reads,
                               rogtk_u32_result* n_distinct) {
    if (int rc = check_correct_outputs(col, representatives, n_reads, n_distinct)) return rc;
    const HostCol h(*col);
    if (int rc = check_host_col(h)) return rc;
    const int64_t n = h.n;
    if (int rc = check_rows_and_clusters("cluster summary", n, n_clusters)) return rc;
    ROGTK_REQUIRE(cluster_id || n == 0, ROGTK_E_INVALID, "cluster_id is NULL");
    for (int64_t i = 0; i < n; ++i)
        ROGTK_REQUIRE(!h.valid(i) || (int64_t)cluster_id[i] < n_clusters, ROGTK_E_INVALID,
                      "cluster_id[%lld] = %u is >= n_clusters (%lld)", (long long)i, cluster_id[i],
                      (long long)n_clusters);
    const int L = umi_len > 0 ? umi_len : h.first_len();
    HostCtx* c;
    if (int rc = host_ctx(&c)) return rc;
    int64_t max_len = 0;
    DevCol dcol(nullptr, h.ow, nullptr, nullptr, h.voff, 0);
    if (n > 0) {
        if (int rc = upload_col(c, 0, h, &dcol)) return rc;
        if (int rc = device_max_len(c, dcol, &max_len)) return rc;
    }
    if (int rc = c->out[0].ensure((size_t)std::max<int64_t>(n, 4) * 4)) return rc;
    if (n > 0)
        if (int rc = c->h2d(c->out[0].p, cluster_id, (size_t)n * 4)) return rc;
    const int rc = summary_to_host(c, dcol, L, c->out[0].as<uint32_t>(), n_clusters, max_len, representatives,
                                   n_reads, n_distinct);
    if (rc) {
        rogtk_str_result_free(representatives);
        rogtk_u32_result_free(n_reads);
        rogtk_u32_result_free(n_distinct);
    }
    return rc;
}

void rogtk_u32_result_free(rogtk_u32_result* r) {
    if (!r) return;
    free(r->data);
    u32_result_reset(r);
}

int rogtk_cluster_summary_dev(const int64_t* offsets, const uint8_t* values, const uint8_t* validity, int64_t n,
                              int umi_len, const uint32_t* cluster_id, int64_t n_clusters, uint32_t* n_reads,
                              uint32_t* n_distinct, int64_t* rep_rows, int64_t* rep_offsets, int64_t* rep_values_len,
                              void* stream) {
    if (int rc = check_rows_and_clusters("cluster_summary_dev", n, n_clusters)) return rc;
    ROGTK_REQUIRE(n == 0 || (offsets && values && cluster_id), ROGTK_E_INVALID, "cluster_summary_dev: NULL input");
    ROGTK_REQUIRE(n_reads && n_distinct && rep_rows && rep_offsets && rep_values_len, ROGTK_E_INVALID,
                  "cluster_summary_dev: NULL output");
    ROGTK_REQUIRE(umi_len >= 1, ROGTK_E_INVALID, "cluster_summary_dev: umi_len must be >= 1");
    *rep_values_len = 0;
    hipStream_t s = as_stream(stream);
    HostCtx* c;
    if (int rc = host_ctx(&c)) return rc;
    const DevCol col(offsets, values, validity, n);
    int64_t max_len = 0;
    if (n > 0) {
        if (int rc = c->nirr.ensure(16)) return rc;
        if (int rc = column_max_len(offsets, 8, n, c->nirr.as<unsigned long long>() + 1, s, &max_len)) return rc;
    }
    if (int rc = cluster_summary_general(col, umi_len, cluster_id, n_clusters, max_len, n_reads, n_distinct, rep_rows,
                                         s))
        return rc;
    int64_t tb = 0;
    if (int rc = representatives_temp(n_clusters, &tb)) return rc;
    if (int rc = c->out[5].ensure((size_t)tb)) return rc;
    if (int rc = representatives_measure(col, rep_rows, n_clusters, rep_offsets, c->out[5].p, tb, s)) return rc;
    ROGTK_HIP_CHECK(hipMemcpyAsync(rep_values_len, rep_offsets + n_clusters, 8, hipMemcpyDeviceToHost, s));
    ROGTK_HIP_CHECK(hipStreamSynchronize(s));
    return ROGTK_OK;
}

int rogtk_cluster_representatives_fill(const int64_t* offsets, const uint8_t* values, const int64_t* rep_rows,
                                       int64_t n_clusters, const int64_t* rep_offsets, uint8_t* rep_values,
                                       void* stream) {
    ROGTK_REQUIRE(n_clusters >= 0, ROGTK_E_INVALID, "representatives_fill: negative n_clusters");
    ROGTK_REQUIRE(n_clusters == 0 || (offsets && values && rep_rows && rep_offsets && rep_values), ROGTK_E_INVALID,
                  "representatives_fill: NULL argument");
    return representatives_fill(offsets, 8, values, rep_rows, n_clusters, rep_offsets, rep_values, as_stream(stream));
}

// ------------------------------------ directional UMI clustering (directional.hip)
int rogtk_directional_temp_bytes(int64_t m, int umi_len, int64_t* bytes) {
    ROGTK_REQUIRE(bytes, ROGTK_E_INVALID, "directional_temp_bytes: NULL bytes");
    ROGTK_REQUIRE(umi_len >= 1 && umi_len <= 32, ROGTK_E_UNSUPPORTED, "directional: umi_len %d outside 1..32", umi_len);
    ROGTK_REQUIRE(m >= 0 && m < (1ll << 31), ROGTK_E_UNSUPPORTED, "directional: m %lld outside 0..2^31-1",
                  (long long)m);
    return directional_codes_temp(m, umi_len, bytes);
}

int rogtk_directional_codes(const uint64_t* codes, const uint32_t* counts, int64_t m, int umi_len, uint32_t* root,
                            uint32_t* labels, int64_t* n_clusters, int64_t* rounds, void* temp, int64_t temp_bytes,
                            void* stream) {
    ROGTK_REQUIRE(umi_len >= 1 && umi_len <= 32, ROGTK_E_UNSUPPORTED, "directional: umi_len %d outside 1..32", umi_len);
    ROGTK_REQUIRE(m >= 0 && m < (1ll << 31), ROGTK_E_UNSUPPORTED, "directional: m %lld outside 0..2^31-1",
                  (long long)m);
    ROGTK_REQUIRE(n_clusters && rounds, ROGTK_E_INVALID, "directional: NULL n_clusters / rounds");
    ROGTK_REQUIRE(m == 0 || (codes && counts && root && labels && temp), ROGTK_E_INVALID, "directional: NULL argument");
    const int rc = directional_codes(codes, counts, m, umi_len, root, labels, n_clusters, rounds, temp, temp_bytes,
                                     as_stream(stream));
    t_directional_rounds = *rounds;
    return rc;
}

int rogtk_directional_last_rounds(int64_t* rounds) {
    ROGTK_REQUIRE(rounds, ROGTK_E_INVALID, "directional_last_rounds: NULL rounds");
    *rounds = t_directional_rounds;
    return ROGTK_OK;
}

int rogtk_umi_cluster_directional_host(const void* offsets, int offset_width, const uint8_t* values, int64_t values_len,
                                       const uint8_t* validity, int64_t validity_offset, int64_t n, int umi_len,
                                       int max_distance, uint32_t* cluster_id, int64_t* n_clusters,
                                       int* resolved_umi_len) {
    // max_distance 0 is rogtk_umi_cluster_host's call, which has no row limit
    return cluster_host("umi_cluster_directional",
                        HostCol(offsets, offset_width, values, values_len, validity, validity_offset, n), umi_len,
                        ClusterRule{1, max_distance, nullptr},
                        (max_distance == 0 ? 0u : kRowLimit) | null_arg(cluster_id || n == 0), cluster_id, n_clusters,
                        resolved_umi_len, nullptr);
}

int rogtk_umi_cluster_directional_dev(const int64_t* offsets, const uint8_t* values, const uint8_t* validity, int64_t n,
                                      int umi_len, uint32_t* cluster_id, int64_t* n_clusters, uint64_t* root_code,
                                      void* stream) {
    const ClusterRule rule{1, 1, nullptr};
    if (int rc = check_cluster_call("umi_cluster_directional_dev", n, umi_len, rule,
                                    kRowLimit | kDeviceCol | null_arg(n == 0 || (offsets && values && cluster_id))))
        return rc;
    return ids_dev(DevCol(offsets, values, validity, n), umi_len, rule, ClusterIds{cluster_id, root_code}, n_clusters,
                   nullptr, as_stream(stream));
}

int rogtk_umi_correct_directional_host(const rogtk_str_col* col, int umi_len, int max_distance, uint32_t* cluster_id,
                                       rogtk_str_result* corrected, rogtk_str_result* representatives,
                                       rogtk_u32_result* n_reads, rogtk_u32_result* n_distinct, int64_t* n_clusters,
                                       int* resolved_umi_len) {
    return correct_host("umi_correct_directional", col, umi_len, ClusterRule{1, max_distance, nullptr}, 0, cluster_id,
                        corrected, representatives, n_reads, n_distinct, nullptr, n_clusters, resolved_umi_len);
}

int rogtk_umi_correct_directional_dev(const int64_t* offsets, const uint8_t* values, const uint8_t* validity, int64_t n,
                                      int umi_len, uint32_t* cluster_id, int64_t* n_clusters,
                                      uint8_t* corrected_values, void* stream) {
    const ClusterRule rule{1, 1, nullptr};
    if (int rc = check_cluster_call("umi_correct_directional_dev", n, umi_len, rule,
                                    kRowLimit | kDeviceCol |
                                        null_arg(n == 0 || (offsets && values && cluster_id && corrected_values))))
        return rc;
    return ids_dev(DevCol(offsets, values, validity, n), umi_len, rule, ClusterIds{cluster_id}, n_clusters,
                   corrected_values, as_stream(stream));
}

// ------------------------------------ clustering within groups (grouped.hip)
int rogtk_grouped_set_window(int window) { return grouped_set_window(window); }

int rogtk_umi_cluster_grouped_host(const void* offsets, int offset_width, const uint8_t* values, int64_t values_len,
                                   const uint8_t* validity, int64_t validity_offset, int64_t n,
                                   const uint32_t* groups, int umi_len, int method, int max_distance,
                                   uint32_t* cluster_id, int64_t* n_clusters, int* resolved_umi_len,
                                   rogtk_u32_result* cluster_group) {
    return cluster_host("umi_cluster_grouped",
                        HostCol(offsets, offset_width, values, values_len, validity, validity_offset, n), umi_len,
                        grouped_rule(method, max_distance, groups),
                        kRowLimit | kGrouped | null_arg((cluster_id && groups) || n == 0), cluster_id, n_clusters,
                        resolved_umi_len, cluster_group);
}

int rogtk_umi_cluster_grouped_dev(const int64_t* offsets, const uint8_t* values, const uint8_t* validity, int64_t n,
                                  const uint32_t* groups, int umi_len, int method, int max_distance,
                                  uint32_t* cluster_id, int64_t* n_clusters, uint64_t* root_code,
                                  uint32_t* cluster_group, void* stream) {
    const ClusterRule rule = grouped_rule(method, max_distance, groups);
    if (int rc = check_cluster_call("umi_cluster_grouped_dev", n, umi_len, rule,
                                    kRowLimit | kGrouped | kDeviceCol |
                                        null_arg(n == 0 || (offsets && values && cluster_id && groups))))
        return rc;
    return ids_dev(DevCol(offsets, values, validity, n), umi_len, rule,
                   ClusterIds{cluster_id, root_code, cluster_group}, n_clusters, nullptr, as_stream(stream));
}

int rogtk_umi_correct_grouped_host(const rogtk_str_col* col, const uint32_t* groups, int umi_len, int method,
                                   int max_distance, uint32_t* cluster_id, rogtk_str_result* corrected,
                                   rogtk_str_result* representatives, rogtk_u32_result* n_reads,
                                   rogtk_u32_result* n_distinct, rogtk_u32_result* cluster_group,
                                   int64_t* n_clusters, int* resolved_umi_len) {
    return correct_host("umi_correct_grouped", col, umi_len, grouped_rule(method, max_distance, groups),
                        kGrouped | null_arg(groups || !col || col->n == 0), cluster_id, corrected, representatives,
                        n_reads, n_distinct, cluster_group, n_clusters, resolved_umi_len);
}

int rogtk_umi_correct_grouped_dev(const int64_t* offsets, const uint8_t* values, const uint8_t* validity, int64_t n,
                                  const uint32_t* groups, int umi_len, int method, int max_distance,
                                  uint32_t* cluster_id, int64_t* n_clusters, uint8_t* corrected_values,
                                  uint32_t* cluster_group, void* stream) {
    const ClusterRule rule = grouped_rule(method, max_distance, groups);
    if (int rc = check_cluster_call("umi_correct_grouped_dev", n, umi_len, rule,
                                    kRowLimit | kGrouped | kDeviceCol |
                                        null_arg(n == 0 || (offsets && values && cluster_id && corrected_values &&
                                                            groups))))
        return rc;
    return ids_dev(DevCol(offsets, values, validity, n), umi_len, rule, ClusterIds{cluster_id, nullptr, cluster_group},
                   n_clusters, corrected_values, as_stream(stream));
}

}  // extern "C"
