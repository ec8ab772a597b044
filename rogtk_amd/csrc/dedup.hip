// dedup.hip — UMI deduplication on gfx950: per cluster id the row to keep
// (largest score, on a tie the smallest row index), its score and the cluster's row count;
// per row one bit of an Arrow bitmap that says whether it is the kept row; and the kept rows
// in ascending order.
//
//   cluster_id[n] u32, score[n] u32 (absent: every score 0), n_clusters; a row whose id is
//   >= n_clusters (0xFFFFFFFF, the null row, among them) is skipped: never kept, never counted.
//
// Every row has one u64 key, score << 32 | (0xFFFFFFFF - row). row < 2^31, so a key is never
// 0 and 0 means "no row"; the largest key of a cluster is its (score descending, row
// ascending) winner, and keys are distinct, so exactly one row per non-empty cluster wins.
//
//   select   votes[id] = max key, n_reads[id] = rows. A workgroup takes kSelTile consecutive
//            rows, 16 bytes of ids and of scores per lane and step, and combines them in an LDS
//            table hashed by id (slot = id * 2654435761 >> (32 - log2 kSlots), kProbes linear
//            probes, slots claimed by atomicCAS on the id; a row that finds no slot goes
//            straight to the global tables) before one global atomicMax + atomicAdd per used
//            slot. When every live row of a wave's step has the same id, the wave reduces key
//            and count in registers and issues one LDS update (sorted ids, the giant cluster).
//   keep     each lane re-forms its key and compares it with votes[id]; the ballot of a wave
//            is the 64-row keep word (rows past n and skipped rows give 0, so the padding bits
//            are written as zero); a workgroup also leaves the popcount of its kKeepTile rows.
//   compact  exclusive scan of the tile popcounts (k_tile_scan of id_columns.h), then a scatter
//            of the set bits of every tile, ascending by construction.
//   decode   votes[c] -> best_row[c] (-1 without rows), best_score[c].
//
// max and add commute, so the answer does not depend on geometry or scheduling. Enqueue-only:
// no allocation, no synchronisation, everything on the caller's stream.
#include <atomic>

#include "../../include/rogtk_dedup.h"
#include "id_columns.h"

namespace rogtk {
namespace {

constexpr int kBlock = 256;
constexpr int kSelSteps = 4;                      // 16-byte loads per lane and tile
constexpr int kSelTile = kBlock * 4 * kSelSteps;  // 4096 rows
constexpr int kSlotBits = 11;
constexpr int kSlots = 1 << kSlotBits;  // 32 KiB of LDS
constexpr int kProbes = 4;
constexpr int kKeepTile = 64 * 64;  // 64 keep words: one lane of wave 0 per word in the scatter
constexpr uint32_t kNoId = 0xFFFFFFFFu;

std::atomic<int> g_combine{1};  // 0: one global atomic per row (measurements only)
std::atomic<int> g_phases{7};   // 1 select | 2 keep + decode | 4 compaction (measurements only)

struct BestShared {
    unsigned long long key[kSlots];
    uint32_t id[kSlots];
    uint32_t rows[kSlots];
};

__device__ __forceinline__ unsigned long long best_key(uint32_t score, int64_t row) {
    return ((unsigned long long)score << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)row);
}

__device__ __forceinline__ void vote_global(unsigned long long* __restrict__ votes, uint32_t* __restrict__ n_reads,
                                            uint32_t id, unsigned long long key, uint32_t rows) {
    atomicMax(&votes[id], key);
    if (n_reads) atomicAdd(&n_reads[id], rows);
}

__device__ __forceinline__ void vote(BestShared& sh, unsigned long long* __restrict__ votes,
                                     uint32_t* __restrict__ n_reads, uint32_t id, unsigned long long key,
                                     uint32_t rows) {
    const uint32_t h = (id * 2654435761u) >> (32 - kSlotBits);
    for (int p = 0; p < kProbes; ++p) {
        const uint32_t slot = (h + p) & (kSlots - 1);
        const uint32_t old = atomicCAS(&sh.id[slot], kNoId, id);
        if (old == kNoId || old == id) {
            atomicMax(&sh.key[slot], key);
            atomicAdd(&sh.rows[slot], rows);
            return;
        }
    }
    vote_global(votes, n_reads, id, key, rows);
}

template <bool COMBINE>
__global__ void __launch_bounds__(kBlock)
k_best_select(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ score, int64_t n, uint32_t nc, bool vec,
              unsigned long long* __restrict__ votes, uint32_t* __restrict__ n_reads) {
    __shared__ BestShared sh;
    if (COMBINE) {
        for (int i = threadIdx.x; i < kSlots; i += kBlock) {
            sh.key[i] = 0ull;
            sh.id[i] = kNoId;
            sh.rows[i] = 0u;
        }
        __syncthreads();
    }
    const int64_t tile = (int64_t)blockIdx.x * kSelTile;
    const int lane = threadIdx.x & 63;
    for (int step = 0; step < kSelSteps; ++step) {
        const int64_t r0 = tile + ((int64_t)step * kBlock + threadIdx.x) * 4;
        uint32_t id[4], sc[4] = {0u, 0u, 0u, 0u};
        load4(ids, r0, n, vec, kNoId, id);
        if (score) load4(score, r0, n, vec, 0u, sc);
        bool ok[4];
        unsigned long long key[4];
        for (int k = 0; k < 4; ++k) {
            ok[k] = r0 + k < n && id[k] < nc;
            key[k] = best_key(sc[k], r0 + k);
        }
        if (!COMBINE) {
            for (int k = 0; k < 4; ++k)
                if (ok[k]) vote_global(votes, n_reads, id[k], key[k], 1u);
            continue;
        }
        const uint64_t live = __ballot(ok[0] || ok[1] || ok[2] || ok[3]);
        if (!live) continue;  // the whole wave: past n or skipped
        const uint32_t mine = ok[0] ? id[0] : ok[1] ? id[1] : ok[2] ? id[2] : id[3];
        const uint32_t first = __shfl(mine, __ffsll((unsigned long long)live) - 1);
        bool same = true;
        for (int k = 0; k < 4; ++k) same = same && (!ok[k] || id[k] == first);
        if (__ballot(!same) == 0) {  // one id in the wave's 256 rows: reduce in registers
            unsigned long long m = 0ull;
            uint32_t c = 0u;
            for (int k = 0; k < 4; ++k)
                if (ok[k]) {
                    m = key[k] > m ? key[k] : m;
                    ++c;
                }
            for (int d = 32; d; d >>= 1) {
                const unsigned long long om = __shfl_xor(m, d);
                m = om > m ? om : m;
                c += __shfl_xor(c, d);
            }
            if (lane == 0) vote(sh, votes, n_reads, first, m, c);
        } else {
            for (int k = 0; k < 4; ++k)
                if (ok[k]) vote(sh, votes, n_reads, id[k], key[k], 1u);
        }
    }
    if (COMBINE) {
        __syncthreads();
        for (int i = threadIdx.x; i < kSlots; i += kBlock) {
            const uint32_t id = sh.id[i];
            if (id != kNoId) vote_global(votes, n_reads, id, sh.key[i], sh.rows[i]);
        }
    }
}

__global__ void __launch_bounds__(kBlock)
k_best_keep(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ score, int64_t n, uint32_t nc,
            const unsigned long long* __restrict__ votes, uint64_t* __restrict__ keep_bits,
            uint32_t* __restrict__ tile_counts) {
    __shared__ uint32_t wsum[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w0 = (int64_t)blockIdx.x * (kKeepTile / 64);
    uint32_t cnt = 0;
    for (int j = wave; j < kKeepTile / 64; j += kBlock / 64) {
        const int64_t w = w0 + j;
        if (w * 64 >= n) break;  // the whole wave
        const int64_t i = w * 64 + lane;
        bool keep = false;
        if (i < n) {
            const uint32_t id = stream_load(ids + i);
            if (id < nc) keep = votes[id] == best_key(score ? stream_load(score + i) : 0u, i);
        }
        const uint64_t word = __ballot(keep);
        if (lane == 0) keep_bits[w] = word;
        cnt += (uint32_t)__popcll(word);
    }
    if (!tile_counts) return;
    if (lane == 0) wsum[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int k = 0; k < kBlock / 64; ++k) t += wsum[k];
        tile_counts[blockIdx.x] = t;
    }
}

// the set bits of one tile's 64 keep words, ascending, from the tile's offset on
__global__ void __launch_bounds__(kBlock)
k_best_scatter(const uint64_t* __restrict__ keep_bits, int64_t n_words, const uint32_t* __restrict__ offs, int64_t cap,
               int64_t* __restrict__ kept_rows) {
    static_assert(kKeepTile == 64 * 64, "one lane of wave 0 per word of the tile");
    __shared__ uint64_t words[64];
    __shared__ uint32_t pre[64];
    const int lane = threadIdx.x & 63;
    const int64_t w0 = (int64_t)blockIdx.x * 64;
    if (threadIdx.x < 64) {
        const int64_t w = w0 + lane;
        const uint64_t word = w < n_words ? keep_bits[w] : 0ull;
        const uint32_t c = (uint32_t)__popcll(word);
        words[lane] = word;
        pre[lane] = wave_scan(c, lane) - c;
    }
    __syncthreads();
    const int64_t base = (int64_t)offs[blockIdx.x];
    const uint64_t below = (1ull << lane) - 1ull;
    for (int j = threadIdx.x >> 6; j < 64; j += kBlock / 64) {
        const uint64_t word = words[j];
        if (!((word >> lane) & 1ull)) continue;
        const int64_t p = base + pre[j] + __popcll(word & below);
        if (p < cap) kept_rows[p] = (w0 + j) * 64 + lane;
    }
}

__global__ void k_best_decode(const unsigned long long* __restrict__ votes, int64_t n_clusters,
                              int64_t* __restrict__ best_row, uint32_t* __restrict__ best_score) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= n_clusters) return;
    const unsigned long long v = votes[c];
    best_row[c] = v ? (int64_t)(0xFFFFFFFFu - (uint32_t)v) : -1;
    if (best_score) best_score[c] = (uint32_t)(v >> 32);
}

// one plane of tile popcounts: its offsets, its total = n_kept
constexpr auto k_best_scan = k_tile_scan<1, 0>;

struct BestLayout {
    size_t off_votes, off_counts, off_offs, total;
    int64_t tiles;
};

BestLayout best_layout(int64_t n, int64_t n_clusters) {
    BestLayout p;
    p.tiles = (n + kKeepTile - 1) / kKeepTile;
    Carve c;
    p.off_votes = c.take((size_t)n_clusters * 8);
    p.off_counts = c.take((size_t)p.tiles * 4);
    p.off_offs = c.take((size_t)p.tiles * 4);
    p.total = c.total;
    return p;
}

int64_t cluster_best_temp(int64_t n, int64_t n_clusters) { return (int64_t)best_layout(n, n_clusters).total; }

void cluster_best_geometry(int64_t out[4]) {
    out[0] = kSelTile;
    out[1] = kKeepTile;
    out[2] = kSlots;
    out[3] = kProbes;
}

int cluster_best_set_knobs(int combine, int phases) {
    ROGTK_REQUIRE((combine == 0 || combine == 1) && phases >= 1 && phases <= 7, ROGTK_E_INVALID,
                  "cluster_best knobs: combine %d must be 0 or 1, phases %d a mask in 1..7", combine, phases);
    g_combine.store(combine);
    g_phases.store(phases);
    return ROGTK_OK;
}

// The arguments are checked by the caller (the C entries below): sizes in range, the required pointers
// present, temp 8-byte aligned and large enough, kept_rows given whenever n_kept is and
// min(n, n_clusters) > 0.
int launch_cluster_best_rows(const uint32_t* ids, const uint32_t* score, int64_t n, int64_t n_clusters,
                             int64_t* best_row, uint32_t* best_score, uint32_t* n_reads, uint64_t* keep_bits,
                             int64_t* kept_rows, int64_t* n_kept, void* temp, hipStream_t s) {
    const BestLayout p = best_layout(n, n_clusters);
    uint8_t* t = (uint8_t*)temp;
    unsigned long long* votes = (unsigned long long*)(t + p.off_votes);
    uint32_t* counts = (uint32_t*)(t + p.off_counts);
    uint32_t* offs = (uint32_t*)(t + p.off_offs);
    const uint32_t nc = (uint32_t)n_clusters;  // < 2^32 - 1
    const int phases = g_phases.load();
    const dim3 b(kBlock);
    if (phases & 1) {
        if (n_clusters > 0) {
            ROGTK_HIP_CHECK(hipMemsetAsync(votes, 0, (size_t)n_clusters * 8, s));
            if (n_reads) ROGTK_HIP_CHECK(hipMemsetAsync(n_reads, 0, (size_t)n_clusters * 4, s));
        }
        if (n > 0 && n_clusters > 0) {
            const bool vec = (((uintptr_t)ids | (uintptr_t)score) & 15u) == 0;
            const dim3 g((unsigned)((n + kSelTile - 1) / kSelTile));
            if (g_combine.load())
                hipLaunchKernelGGL(k_best_select<true>, g, b, 0, s, ids, score, n, nc, vec, votes, n_reads);
            else
                hipLaunchKernelGGL(k_best_select<false>, g, b, 0, s, ids, score, n, nc, vec, votes, n_reads);
        }
    }
    if (phases & 2) {
        if (n > 0)
            hipLaunchKernelGGL(k_best_keep, dim3((unsigned)p.tiles), b, 0, s, ids, score, n, nc, votes, keep_bits,
                               n_kept ? counts : (uint32_t*)nullptr);
        if (n_clusters > 0)
            hipLaunchKernelGGL(k_best_decode, dim3(grid_for(n_clusters, kBlock)), b, 0, s, votes, n_clusters, best_row,
                               best_score);
    }
    if ((phases & 4) && n_kept) {
        hipLaunchKernelGGL(k_best_scan, dim3(1), dim3(kScanBlock), 0, s, counts, p.tiles, offs, n_kept);
        if (n > 0 && kept_rows)
            hipLaunchKernelGGL(k_best_scatter, dim3((unsigned)p.tiles), b, 0, s, keep_bits, (n + 63) / 64, offs,
                               std::min(n, n_clusters), kept_rows);
    }
    ROGTK_HIP_CHECK(hipGetLastError());
    return ROGTK_OK;
}

int check_sizes(const char* name, int64_t n, int64_t n_clusters) {
    if (int rc = check_rows(name, n)) return rc;
    ROGTK_REQUIRE(n_clusters >= 0 && n_clusters < (1ll << 32) - 1, ROGTK_E_INVALID,
                  "%s: n_clusters %lld outside 0..2^32-2", name, (long long)n_clusters);
    return ROGTK_OK;
}

// the argument rules of both levels (include/rogtk_dedup.h), before any device work
int check_best(const char* name, const uint32_t* cluster_id, int64_t n, int64_t n_clusters, const int64_t* best_row,
               const uint64_t* keep_bits, const int64_t* kept_rows, const int64_t* n_kept) {
    if (int rc = check_sizes(name, n, n_clusters)) return rc;
    ROGTK_REQUIRE(n == 0 || cluster_id, ROGTK_E_INVALID, "%s: cluster_id is NULL", name);
    ROGTK_REQUIRE(n == 0 || keep_bits, ROGTK_E_INVALID, "%s: keep_bits is NULL", name);
    ROGTK_REQUIRE(n_clusters == 0 || best_row, ROGTK_E_INVALID, "%s: best_row is NULL", name);
    ROGTK_REQUIRE(!kept_rows || n_kept, ROGTK_E_INVALID, "%s: kept_rows without n_kept", name);
    ROGTK_REQUIRE(!n_kept || kept_rows || std::min(n, n_clusters) == 0, ROGTK_E_INVALID,
                  "%s: n_kept without kept_rows", name);
    return ROGTK_OK;
}

}  // namespace
}  // namespace rogtk

// ------------------------------------------------------------------ C ABI
// The entries live in a library of their own, rogtk_amd/_dedup/librogtk_dedup.so.
using namespace rogtk;

extern "C" {

int rogtk_cluster_best_temp_bytes(int64_t n, int64_t n_clusters, int64_t* bytes) {
    ROGTK_REQUIRE(bytes, ROGTK_E_INVALID, "cluster_best_temp_bytes: NULL bytes");
    if (int rc = check_sizes("cluster_best_temp_bytes", n, n_clusters)) return rc;
    *bytes = cluster_best_temp(n, n_clusters);
    return ROGTK_OK;
}

int rogtk_cluster_best_geometry(int64_t* out4) {
    ROGTK_REQUIRE(out4, ROGTK_E_INVALID, "cluster_best_geometry: NULL argument");
    cluster_best_geometry(out4);
    return ROGTK_OK;
}

int rogtk_cluster_best_set_knobs(int combine, int phases) { return cluster_best_set_knobs(combine, phases); }

int rogtk_cluster_best_rows(const uint32_t* cluster_id, const uint32_t* score, int64_t n, int64_t n_clusters,
                            int64_t* best_row, uint32_t* best_score, uint32_t* n_reads, uint64_t* keep_bits,
                            int64_t* kept_rows, int64_t* n_kept, void* temp, int64_t temp_bytes, void* stream) {
    if (int rc = check_best("cluster_best_rows", cluster_id, n, n_clusters, best_row, keep_bits, kept_rows, n_kept))
        return rc;
    const int64_t need = cluster_best_temp(n, n_clusters);
    ROGTK_REQUIRE(temp && ((uintptr_t)temp & 7u) == 0, ROGTK_E_INVALID,
                  "cluster_best_rows: temp is NULL or not 8-byte aligned");
    ROGTK_REQUIRE(temp_bytes >= need, ROGTK_E_INVALID, "cluster_best_rows: temp_bytes %lld too small (need %lld)",
                  (long long)temp_bytes, (long long)need);
    return launch_cluster_best_rows(cluster_id, score, n, n_clusters, best_row, best_score, n_reads, keep_bits,
                                    kept_rows, n_kept, temp, (hipStream_t)stream);
}

int rogtk_cluster_best_rows_host(const uint32_t* cluster_id, const uint32_t* score, int64_t n, int64_t n_clusters,
                                 int64_t* best_row, uint32_t* best_score, uint32_t* n_reads, uint64_t* keep_bits,
                                 int64_t* kept_rows, int64_t* n_kept) {
    if (int rc = check_best("cluster_best_rows_host", cluster_id, n, n_clusters, best_row, keep_bits, kept_rows,
                            n_kept))
        return rc;
    // one allocation, the whole call on the default stream: ids, scores, the outputs, temp
    const int64_t cap = std::min(n, n_clusters), words = (n + 63) / 64;
    HostCall m;
    const size_t o_ids = m.take((size_t)n * 4), o_score = m.take((size_t)n * 4), o_row = m.take((size_t)n_clusters * 8),
                 o_bs = m.take((size_t)n_clusters * 4), o_reads = m.take((size_t)n_clusters * 4),
                 o_keep = m.take((size_t)words * 8), o_kept = m.take((size_t)cap * 8), o_nk = m.take(8),
                 o_temp = m.take((size_t)cluster_best_temp(n, n_clusters));
    if (int rc = m.open("librogtk_dedup")) return rc;
    if (int rc = m.in(o_ids, cluster_id, (size_t)n * 4)) return rc;
    if (int rc = m.in(o_score, score, (size_t)n * 4)) return rc;
    if (int rc = launch_cluster_best_rows(m.at<uint32_t>(o_ids), score ? m.at<uint32_t>(o_score) : nullptr, n,
                                          n_clusters, m.at<int64_t>(o_row), m.at<uint32_t>(o_bs),
                                          m.at<uint32_t>(o_reads), m.at<uint64_t>(o_keep),
                                          n_kept ? m.at<int64_t>(o_kept) : nullptr,
                                          n_kept ? m.at<int64_t>(o_nk) : nullptr, m.at<void>(o_temp), nullptr))
        return rc;
    if (int rc = m.out(best_row, o_row, (size_t)n_clusters * 8)) return rc;
    if (int rc = m.out(best_score, o_bs, (size_t)n_clusters * 4)) return rc;
    if (int rc = m.out(n_reads, o_reads, (size_t)n_clusters * 4)) return rc;
    if (int rc = m.out(keep_bits, o_keep, (size_t)words * 8)) return rc;
    if (!n_kept) return ROGTK_OK;
    if (int rc = m.out(n_kept, o_nk, 8)) return rc;
    ROGTK_REQUIRE(*n_kept >= 0 && *n_kept <= cap, ROGTK_E_HIP, "cluster_best_rows_host: n_kept %lld outside 0..%lld",
                  (long long)*n_kept, (long long)cap);
    return m.out(kept_rows, o_kept, (size_t)*n_kept * 8);
}

}  // extern "C"
