/* rogtk_dedup.h -- C ABI of librogtk_dedup.so (rogtk_amd/csrc/dedup.hip).
 * A companion of rogtk_hip.h: the same status codes, the same error string. */
#ifndef ROGTK_DEDUP_H
#define ROGTK_DEDUP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ====== UMI deduplication: best read per cluster, keep mask, kept rows (dedup.hip) ======
 * The step after clustering that UMI-tools calls dedup: which row stands for each molecule, and
 * which rows are duplicates. These five entries are exported by a library of their own,
 * rogtk_amd/_dedup/librogtk_dedup.so, which links librogtk_hip.so, returns its status codes
 * (rogtk_hip.h) and reports through its error string; load it after librogtk_hip.so.
 *   inputs   cluster_id[n] u32, as every clustering entry writes them (dense 0..n_clusters-1,
 *            0xFFFFFFFF for a null row) or the caller's own; score[n] u32 (MAPQ, summed base
 *            quality, read length ...; NULL: every score is 0); n_clusters. A row whose id is
 *            >= n_clusters is skipped: never kept, never counted.
 *            0 <= n < 2^31, 0 <= n_clusters < 2^32 - 1.
 *   outputs  best_row[n_clusters] int64: the row with the largest score among the rows of the id,
 *            on a tie the smallest row index; -1 for an id without rows.
 *            best_score[n_clusters] u32: that row's score (0 where best_row is -1).
 *            n_reads[n_clusters] u32: the rows of the id.
 *            keep_bits[(n + 63) / 64] u64: bit i % 64 (LSB first) of word i / 64 is set exactly
 *            when best_row[cluster_id[i]] == i: the Arrow bitmap layout. The padding bits of the
 *            last word are zero.
 *            kept_rows[min(n, n_clusters)] int64: the set rows, ascending; entries from *n_kept on
 *            are left untouched. *n_kept: the ids with at least one row.
 * The answer depends on the inputs alone, not on launch geometry or scheduling.
 * Every entry returns ROGTK_E_INVALID before any device work for n or n_clusters out of range,
 * for cluster_id / keep_bits NULL with n > 0, best_row NULL with n_clusters > 0, kept_rows
 * without n_kept, n_kept without kept_rows (unless min(n, n_clusters) is 0), and (Level 1) temp
 * NULL, not 8-byte aligned or temp_bytes too small. With n == 0 the per-cluster outputs are
 * still written (-1 / 0 / 0) and *n_kept = 0. */
int rogtk_cluster_best_temp_bytes(int64_t n, int64_t n_clusters, int64_t* bytes);
/* Level 1, device pointers, enqueue-only (capturable; no sync, no allocation). score,
 * best_score, n_reads, kept_rows and n_kept are nullable (kept_rows and n_kept together).
 * The call initialises what it needs of temp. */
int rogtk_cluster_best_rows(const uint32_t* cluster_id, const uint32_t* score, int64_t n, int64_t n_clusters,
                            int64_t* best_row, uint32_t* best_score, uint32_t* n_reads, uint64_t* keep_bits,
                            int64_t* kept_rows, int64_t* n_kept /* device */, void* temp, int64_t temp_bytes,
                            void* stream);
/* Level 2, host arrays of the same shapes allocated by the caller; n_kept on the host. */
int rogtk_cluster_best_rows_host(const uint32_t* cluster_id, const uint32_t* score, int64_t n, int64_t n_clusters,
                                 int64_t* best_row, uint32_t* best_score, uint32_t* n_reads, uint64_t* keep_bits,
                                 int64_t* kept_rows, int64_t* n_kept);
/* The kernels' constants, for tests at their boundaries: out4 = {rows per select tile, rows per
 * keep / compaction tile, LDS slots of the select table, probes per row}. A row's home slot is
 * (id * 2654435761 mod 2^32) >> (32 - log2 slots). */
int rogtk_cluster_best_geometry(int64_t* out4);
/* Measurements only (process-wide): combine 0 = the select without its LDS combine (one global
 * atomic per row); phases = which parts a call enqueues, 1 select | 2 keep + decode |
 * 4 compaction (the default 7: all; a part alone reads what an earlier full call left in temp
 * and the outputs). The answers of a full call are the same. */
int rogtk_cluster_best_set_knobs(int combine, int phases);

#ifdef __cplusplus
}
#endif
#endif /* ROGTK_DEDUP_H */
