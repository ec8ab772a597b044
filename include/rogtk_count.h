/* rogtk_count.h -- C ABI of librogtk_count.so (rogtk_amd/csrc/count_matrix.hip).
 * A companion of rogtk_hip.h and rogtk_dedup.h: the same status codes, the same error string. */
#ifndef ROGTK_COUNT_H
#define ROGTK_COUNT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ====== The UMI count matrix: molecules and reads per (cell, feature) (count_matrix.hip) ======
 * The table that barcode correction, UMI clustering and deduplication lead to. These entries are
 * exported by a library of their own, rogtk_amd/_count/librogtk_count.so, which links
 * librogtk_hip.so, returns its status codes (rogtk_hip.h) and reports through its error string;
 * load it after librogtk_hip.so.
 *   inputs   cell[n], feature[n], molecule[n] u32; n_cells, n_features, n_molecules, each in
 *            0..2^32-1; 0 <= n < 2^31. A row is live when cell < n_cells, feature < n_features and
 *            molecule < n_molecules; every other row (0xFFFFFFFF, which the barcode keys, a null
 *            gene and a null UMI row's cluster id use, among them) is skipped: counted nowhere.
 *   entries  an entry is a (cell, feature) pair with at least one live row; n_umis is the number of
 *            distinct molecule values among its live rows, n_reads the number of its live rows. A
 *            molecule id under two features or in two cells counts once under each.
 *   outputs  entries ascending in (cell, feature): entry_cell[e], entry_feature[e], n_umis[e],
 *            n_reads[e] u32, e < min(entries, capacity); elements from there on are left untouched.
 *            totals[3] int64: the entries (the true count, also past capacity), the live rows, the
 *            sum of n_umis.
 *            indptr[n_cells + 1] int64 (nullable): indptr[c] = the first written entry whose cell
 *            is >= c, indptr[n_cells] = min(entries, capacity): the CSR row pointer.
 * The key of a row is cell << (fb + mb) | feature << mb | molecule with cb = bit_width(n_cells),
 * fb = bit_width(n_features - 1), mb = bit_width(n_molecules - 1); cb + fb + mb > 64 is
 * ROGTK_E_UNSUPPORTED, decided from the three sizes before any device work (the message names the
 * three widths). The answer depends on the inputs alone, not on launch geometry or scheduling.
 * Every entry returns ROGTK_E_INVALID before any device work for n or a size out of range, a
 * negative capacity (Level 1 and temp_bytes), cell / feature / molecule NULL with n > 0,
 * entry_cell / entry_feature / n_umis NULL with capacity > 0, totals NULL, and (Level 1) temp
 * NULL, temp not 8-byte aligned or temp_bytes too small. With n == 0 or a size of 0 there are no
 * entries: totals = {0, 0, 0} and indptr all 0, still written on the device.
 * temp_bytes includes hipCUB's sort scratch as its size query reports it for the current device;
 * in a machine without a device that query fails and the scratch is estimated instead (12 bytes
 * per row + 1 MiB), which serves to size a request but not a call. */
int rogtk_count_matrix_temp_bytes(int64_t n, int64_t n_cells, int64_t n_features, int64_t n_molecules,
                                  int64_t capacity, int64_t* bytes);
/* Level 1, device pointers, enqueue-only (capturable; no sync, no allocation). n_reads and indptr
 * are nullable. The call initialises what it needs of temp. */
int rogtk_count_matrix(const uint32_t* cell, const uint32_t* feature, const uint32_t* molecule, int64_t n,
                       int64_t n_cells, int64_t n_features, int64_t n_molecules, uint32_t* entry_cell,
                       uint32_t* entry_feature, uint32_t* n_umis, uint32_t* n_reads, int64_t capacity,
                       int64_t* indptr, int64_t* totals /* device */, void* temp, int64_t temp_bytes, void* stream);
/* Level 2, host arrays of the same shapes allocated by the caller; totals on the host.
 * capacity < 0: min(n, n_cells * n_features), which no entry count passes. */
int rogtk_count_matrix_host(const uint32_t* cell, const uint32_t* feature, const uint32_t* molecule, int64_t n,
                            int64_t n_cells, int64_t n_features, int64_t n_molecules, uint32_t* entry_cell,
                            uint32_t* entry_feature, uint32_t* n_umis, uint32_t* n_reads, int64_t capacity,
                            int64_t* indptr, int64_t* totals);
/* The kernels' constants, for tests at their boundaries: out2 = {sorted positions per flag / emit
 * tile, threads of the scan's one workgroup}. */
int rogtk_count_matrix_geometry(int64_t* out2);
/* Measurements only (process-wide): which parts a call enqueues, 1 pack | 2 sort | 4 flags, scan,
 * emit, diff and indptr (the default 7: all; a part alone reads what an earlier full call left
 * in temp). */
int rogtk_count_matrix_set_phases(int phases);

#ifdef __cplusplus
}
#endif
#endif /* ROGTK_COUNT_H */
