// correct.hip — UMI correction on gfx950: per cluster its representative
// UMI (the distinct string with the most rows; ties: regular before irregular, then the
// byte-lexicographically smallest), its read count and its distinct-UMI count; per row
// the representative of its cluster.
//
// Every path is count -> vote -> gather:
//   count   rows per distinct string. Packed (u32 codes, L <= 16): the regular rows'
//           (code, cluster id) pairs are radix-sorted over the 2 L code bits; a run of equal
//           codes is one distinct UMI, and its head thread finds the run's end with a
//           galloping search in the sorted codes (runs are short, the search stays in one
//           or two cache lines; no scan, nothing special where a run crosses a workgroup).
//           General (any strings): rows sorted by (cluster id, byte-lexicographic rank of
//           the string, irregular.hip's string sort), runs found the same way.
//           Alternative kept behind rogtk_cluster_summary_set_method (L <= 12): a u32 count
//           table over the 4^L code space, one scattered atomic per row.
//   vote    one atomicMax per distinct string on a u64 key per cluster,
//           count << 33 | regular << 32 | (0xFFFFFFFF - order), order = the code (packed)
//           or the string's rank (general); one atomicAdd each for n_reads and n_distinct.
//           A workgroup combines its votes per cluster in LDS first (VoteShared).
//   gather  corrected[i] = representative[id[i]], streamed.
#include <hipcub/hipcub.hpp>

#include <atomic>

#include "column_util.h"
#include "level2.h"

namespace rogtk {
namespace {

constexpr int kBlock = 256;
constexpr int kTableMaxLen = 12;  // count-table method: 2 x 4^L x 4 bytes of temp (128 MiB at 12)

std::atomic<int> g_summary_method{0};  // 0 = sort, 1 = count table (L <= kTableMaxLen)


__device__ __forceinline__ unsigned long long vote_key(uint64_t count, bool regular, uint32_t order) {
    return (count << 33) | ((uint64_t)regular << 32) | (uint64_t)(0xFFFFFFFFu - order);
}

// End of the run of `key` that starts at k in sorted[0, m): gallop, then bisect.
template <class K>
__device__ __forceinline__ int64_t run_end(const K* __restrict__ sorted, int64_t k, int64_t m, K key, K mask) {
    int64_t lo = k, step = 1;  // sorted[lo] == key
    while (lo + step < m && (sorted[lo + step] & mask) == key) {
        lo += step;
        step <<= 1;
    }
    int64_t l = lo + 1, h = lo + step < m ? lo + step : m;
    while (l < h) {
        const int64_t mid = (l + h) >> 1;
        if ((sorted[mid] & mask) == key) l = mid + 1;
        else h = mid;
    }
    return l;
}

// Votes of one workgroup, combined in LDS before they reach the per-cluster tables. A
// Hamming-1 graph of real UMIs has a giant component (synth-v1 at the C2 shape: ~0.9 M of
// the 1.08 M distinct codes in one cluster), and one global atomic per distinct code on
// that cluster's three words serialises (measured: 11.4 ms for 10 M rows). A workgroup
// covers kTile consecutive sorted rows, hashes each vote's cluster id into kSlots LDS
// slots (linear probing, a few probes; a vote that finds no slot goes straight to the
// global tables) and flushes each used slot with one set of global atomics.
constexpr int kRowsPerThread = 16;
constexpr int kTile = kBlock * kRowsPerThread;
constexpr int kSlots = 1024;
constexpr int kProbes = 8;
struct VoteShared {
    unsigned long long key[kSlots];
    uint32_t id[kSlots];
    uint32_t reads[kSlots];
    uint32_t distinct[kSlots];
};
struct VoteTables {
    unsigned long long* votes;
    uint32_t* n_reads;
    uint32_t* n_distinct;
};
__device__ __forceinline__ void votes_init(VoteShared& sh) {
    for (int i = threadIdx.x; i < kSlots; i += kBlock) {
        sh.key[i] = 0ull;
        sh.id[i] = 0xFFFFFFFFu;
        sh.reads[i] = 0u;
        sh.distinct[i] = 0u;
    }
    __syncthreads();
}
__device__ __forceinline__ void vote(VoteShared& sh, const VoteTables& t, uint32_t id, unsigned long long key,
                                     uint32_t count) {
    const uint32_t h = (id * 2654435761u) >> 22;
    for (int p = 0; p < kProbes; ++p) {
        const uint32_t slot = (h + p) & (kSlots - 1);
        const uint32_t old = atomicCAS(&sh.id[slot], 0xFFFFFFFFu, id);
        if (old == 0xFFFFFFFFu || old == id) {
            atomicMax(&sh.key[slot], key);
            atomicAdd(&sh.reads[slot], count);
            atomicAdd(&sh.distinct[slot], 1u);
            return;
        }
    }
    atomicMax(&t.votes[id], key);
    atomicAdd(&t.n_reads[id], count);
    atomicAdd(&t.n_distinct[id], 1u);
}
__device__ __forceinline__ void votes_flush(VoteShared& sh, const VoteTables& t) {
    __syncthreads();
    for (int i = threadIdx.x; i < kSlots; i += kBlock) {
        const uint32_t id = sh.id[i];
        if (id == 0xFFFFFFFFu) continue;
        atomicMax(&t.votes[id], sh.key[i]);
        atomicAdd(&t.n_reads[id], sh.reads[i]);
        atomicAdd(&t.n_distinct[id], sh.distinct[i]);
    }
}
inline unsigned tiles_for(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + kTile - 1) / kTile); }

// ------------------------------------------------------------------ packed
// Regular rows' (code, id) pairs to the front of key / val, the other rows' slots (largest
// key, id 0xFFFFFFFF) from the back, so that a stable sort leaves the m = cnt[0] regular
// pairs in [0, m). A workgroup takes kTile rows = 64 words of regular bits: wave 0 scans
// their popcounts and reserves the tile's two ranges with one atomic each (one atomic per
// wave on the same counter measured 1.9 ms for 10 M rows), then a row's slot is its word's
// prefix + the set bits below its own.
__global__ void __launch_bounds__(kBlock)
k_pack_regular(const uint32_t* __restrict__ codes, const uint64_t* __restrict__ regbits,
               const uint32_t* __restrict__ ids, int64_t n, uint32_t mask, uint32_t* __restrict__ key,
               uint32_t* __restrict__ val, unsigned long long* __restrict__ cnt) {
    static_assert(kTile == 64 * 64, "one lane of wave 0 per word of the tile");
    __shared__ uint64_t words[64];
    __shared__ uint32_t pre_r[64], pre_i[64];
    __shared__ unsigned long long base[2];
    const int64_t tile = (int64_t)blockIdx.x * kTile;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < 64) {
        const int64_t first = tile + 64 * (int64_t)lane;  // first row of this lane's word
        uint64_t live = 0, word = 0;
        if (first < n) {
            live = n - first >= 64 ? ~0ull : (1ull << (n - first)) - 1ull;
            word = regbits[first >> 6] & live;
        }
        const uint32_t cr = (uint32_t)__popcll(word), ci = (uint32_t)__popcll(live & ~word);
        uint32_t sr = cr, si = ci;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t ur = __shfl_up(sr, d), ui = __shfl_up(si, d);
            if (lane >= d) {
                sr += ur;
                si += ui;
            }
        }
        words[lane] = word;
        pre_r[lane] = sr - cr;
        pre_i[lane] = si - ci;
        if (lane == 63) {
            base[0] = sr ? atomicAdd(&cnt[0], (unsigned long long)sr) : 0ull;
            base[1] = si ? atomicAdd(&cnt[1], (unsigned long long)si) : 0ull;
        }
    }
    __syncthreads();
    const uint64_t below = (1ull << lane) - 1ull;
    for (int j = threadIdx.x >> 6; j < 64; j += kBlock / 64) {
        const int64_t i = tile + 64 * (int64_t)j + lane;
        if (i >= n) continue;
        const uint64_t word = words[j];
        if ((word >> lane) & 1ull) {
            const int64_t p = (int64_t)base[0] + pre_r[j] + __popcll(word & below);
            key[p] = stream_load(codes + i) & mask;
            val[p] = stream_load(ids + i);
        } else {
            const int64_t p = n - 1 - ((int64_t)base[1] + pre_i[j] + __popcll(~word & below));
            key[p] = mask;
            val[p] = 0xFFFFFFFFu;
        }
    }
}

// Head of each run of equal codes in the sorted pairs: one vote for its cluster.
__global__ void __launch_bounds__(kBlock)
k_vote_runs(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val, int64_t n,
            const unsigned long long* __restrict__ cnt, uint32_t mask, int64_t n_clusters, VoteTables t) {
    __shared__ VoteShared sh;
    votes_init(sh);
    const int64_t m = cnt ? (int64_t)cnt[0] : n;
    const int64_t base = (int64_t)blockIdx.x * kTile;
    for (int r = 0; r < kRowsPerThread; ++r) {
        const int64_t k = base + (int64_t)r * kBlock + threadIdx.x;
        if (k >= m) continue;
        const uint32_t code = key[k] & mask;
        if (k > 0 && (key[k - 1] & mask) == code) continue;
        const uint32_t id = val[k];
        if ((int64_t)id >= n_clusters) continue;
        const uint64_t count = (uint64_t)(run_end<uint32_t>(key, k, m, code, mask) - k);
        vote(sh, t, id, vote_key(count, true, code), (uint32_t)count);
    }
    votes_flush(sh, t);
}

// count-table method: one scattered atomic per regular row ...
__global__ void k_table_count(const uint32_t* __restrict__ codes, const uint64_t* __restrict__ regbits,
                              const uint32_t* __restrict__ ids, int64_t n, uint32_t mask,
                              uint32_t* __restrict__ tab, uint32_t* __restrict__ idtab) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (regbits && !((regbits[i >> 6] >> (i & 63)) & 1ull)) return;
    const uint32_t code = stream_load(codes + i) & mask;
    atomicAdd(&tab[code], 1u);
    idtab[code] = stream_load(ids + i);
}
// ... then one vote per present code of the 4^L code space
__global__ void __launch_bounds__(kBlock)
k_table_vote(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ idtab, int64_t space, int64_t n_clusters,
             VoteTables t) {
    __shared__ VoteShared sh;
    votes_init(sh);
    const int64_t base = (int64_t)blockIdx.x * kTile;
    for (int r = 0; r < kRowsPerThread; ++r) {
        const int64_t c = base + (int64_t)r * kBlock + threadIdx.x;
        if (c >= space) continue;
        const uint32_t count = tab[c];
        if (!count) continue;
        const uint32_t id = idtab[c];
        if ((int64_t)id >= n_clusters) continue;
        vote(sh, t, id, vote_key(count, true, (uint32_t)c), count);
    }
    votes_flush(sh, t);
}

__global__ void k_rep_codes(const unsigned long long* __restrict__ votes, int64_t n_clusters,
                            uint32_t* __restrict__ rep_code) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= n_clusters) return;
    const unsigned long long v = votes[c];
    rep_code[c] = v ? 0xFFFFFFFFu - (uint32_t)v : 0xFFFFFFFFu;  // no regular row: 0xFFFFFFFF
}

// corrected[i] = rep_code[id[i]]; 4 rows per thread (they share one word of regular bits)
__global__ void k_correct4(const uint32_t* __restrict__ ids, const uint64_t* __restrict__ regbits, int64_t n4,
                           const uint32_t* __restrict__ rep_code, uint32_t nc, uint32_t* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= n4) return;
    const u32x4_t id = stream_load((const u32x4_t*)ids + q);
    const uint32_t bits = regbits ? (uint32_t)((regbits[q >> 4] >> ((q & 15) * 4)) & 15ull) : 15u;
    u32x4_t o;
    o.x = (bits & 1u) && id.x < nc ? rep_code[id.x] : 0xFFFFFFFFu;
    o.y = (bits & 2u) && id.y < nc ? rep_code[id.y] : 0xFFFFFFFFu;
    o.z = (bits & 4u) && id.z < nc ? rep_code[id.z] : 0xFFFFFFFFu;
    o.w = (bits & 8u) && id.w < nc ? rep_code[id.w] : 0xFFFFFFFFu;
    stream_store(o, (u32x4_t*)out + q);
}
__global__ void k_correct1(const uint32_t* __restrict__ ids, const uint64_t* __restrict__ regbits, int64_t i0,
                           int64_t n, const uint32_t* __restrict__ rep_code, uint32_t nc, uint32_t* __restrict__ out) {
    const int64_t i = i0 + (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const bool reg = !regbits || ((regbits[i >> 6] >> (i & 63)) & 1ull);
    const uint32_t id = ids[i];
    out[i] = reg && id < nc ? rep_code[id] : 0xFFFFFFFFu;
}

struct PackedLayout {
    size_t off_cnt, off_votes, off_key[2], off_val[2], off_sort, sort_bytes, off_tab, off_idtab, total;
};

int packed_layout(int64_t n, int L, int64_t n_clusters, PackedLayout* p) {
    size_t sb = 0;
    ROGTK_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, sb, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                       (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                       (int)std::max<int64_t>(n, 1), 0, 2 * L));
    Carve c;
    p->off_cnt = c.take(16);
    p->off_votes = c.take((size_t)n_clusters * 8);
    for (int k = 0; k < 2; ++k) p->off_key[k] = c.take((size_t)n * 4);
    for (int k = 0; k < 2; ++k) p->off_val[k] = c.take((size_t)n * 4);
    p->sort_bytes = sb;
    p->off_sort = c.take(sb);
    p->off_tab = p->off_idtab = 0;
    if (L <= kTableMaxLen) {
        p->off_tab = c.take((size_t)4 << (2 * L));
        p->off_idtab = c.take((size_t)4 << (2 * L));
    }
    p->total = c.total;
    return ROGTK_OK;
}

// ----------------------------------------------------------------- general
// the non-null rows, in any order (wave-aggregated append); flags an id >= n_clusters
__global__ void k_valid_rows(const uint8_t* __restrict__ validity, int64_t voff, int64_t n,
                             const uint32_t* __restrict__ ids, int64_t n_clusters, int64_t* __restrict__ rows,
                             unsigned long long* __restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool ok = i < n && row_valid(validity, voff, i);
    if (ok && (int64_t)ids[i] >= n_clusters) cnt[1] = 1ull;
    const uint64_t m = __ballot(ok);
    if (!m) return;
    const int lane = threadIdx.x & 63;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&cnt[0], (unsigned long long)__popcll(m));
    base = __shfl(base, 0);
    if (ok) rows[base + __popcll(m & ((1ull << lane) - 1ull))] = i;
}

__global__ void k_pair_keys(const int64_t* __restrict__ rows, int64_t m, const uint32_t* __restrict__ ids,
                            const uint32_t* __restrict__ srank, uint64_t* __restrict__ key,
                            uint32_t* __restrict__ val) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= m) return;
    const int64_t r = rows[k];
    key[k] = ((uint64_t)ids[r] << 32) | (uint64_t)srank[r];
    val[k] = (uint32_t)r;
}

// sorted by (id, string rank): the head of each run is one distinct string of one cluster
template <int OW>
__global__ void __launch_bounds__(kBlock)
k_vote_strings(const void* __restrict__ offs, const uint8_t* __restrict__ vals, const uint64_t* __restrict__ key,
               const uint32_t* __restrict__ row, int64_t m, int L, VoteTables t) {
    __shared__ VoteShared sh;
    votes_init(sh);
    const int64_t base = (int64_t)blockIdx.x * kTile;
    for (int r = 0; r < kRowsPerThread; ++r) {
        const int64_t k = base + (int64_t)r * kBlock + threadIdx.x;
        if (k >= m) continue;
        const uint64_t kk = key[k];
        if (k > 0 && key[k - 1] == kk) continue;
        const uint64_t count = (uint64_t)(run_end<uint64_t>(key, k, m, kk, ~0ull) - k);
        int64_t st, len;
        span<OW>(offs, (int64_t)row[k], st, len);
        bool regular = L >= 1 && L <= 32 && len == L;
        for (int64_t j = 0; regular && j < len; ++j) {
            const uint8_t b = vals[st + j];
            regular = b == 'A' || b == 'C' || b == 'G' || b == 'T';
        }
        vote(sh, t, (uint32_t)(kk >> 32), vote_key(count, regular, (uint32_t)kk), (uint32_t)count);
    }
    votes_flush(sh, t);
}

// the run whose rank won its cluster's vote names the representative row (ranks are
// distinct within a cluster, so exactly one run writes)
__global__ void k_pick_rows(const uint64_t* __restrict__ key, const uint32_t* __restrict__ row, int64_t m,
                            const unsigned long long* __restrict__ votes, int64_t* __restrict__ rep_row) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= m) return;
    const uint64_t kk = key[k];
    if (k > 0 && key[k - 1] == kk) return;
    const uint32_t id = (uint32_t)(kk >> 32);
    if (0xFFFFFFFFu - (uint32_t)votes[id] == (uint32_t)kk) rep_row[id] = (int64_t)row[k];
}

template <int OW>
__global__ void k_rep_lengths(const void* __restrict__ offs, const int64_t* __restrict__ rep_row, int64_t nc,
                              int64_t* __restrict__ lengths) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c > nc) return;
    int64_t st = 0, len = 0;
    if (c < nc && rep_row[c] >= 0) span<OW>(offs, rep_row[c], st, len);
    lengths[c] = len;
}

template <int OW>
__global__ void k_rep_fill(const void* __restrict__ offs, const uint8_t* __restrict__ vals,
                           const int64_t* __restrict__ rep_row, int64_t nc, const int64_t* __restrict__ out_offs,
                           uint8_t* __restrict__ out) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= nc || rep_row[c] < 0) return;
    int64_t st, len;
    span<OW>(offs, rep_row[c], st, len);
    const int64_t room = out_offs[c + 1] - out_offs[c];
    if (len > room) len = room;
    uint8_t* o = out + out_offs[c];
    for (int64_t j = 0; j < len; ++j) o[j] = vals[st + j];
}

// corrected values under the input's own offsets (every member of a cluster has its
// representative's byte length: ids computed by the library)
template <int OW>
__global__ void k_corrected_fill(const void* __restrict__ offs, const uint8_t* __restrict__ vals,
                                 const uint8_t* __restrict__ validity, int64_t voff, int64_t n,
                                 const uint32_t* __restrict__ ids, int64_t n_clusters,
                                 const int64_t* __restrict__ rep_row, uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || !row_valid(validity, voff, i)) return;
    const uint32_t id = ids[i];
    if ((int64_t)id >= n_clusters) return;
    const int64_t r = rep_row[id];
    if (r < 0) return;
    int64_t st, len, rs, rl;
    span<OW>(offs, i, st, len);
    span<OW>(offs, r, rs, rl);
    if (len > rl) len = rl;
    for (int64_t j = 0; j < len; ++j) out[st + j] = vals[rs + j];
}

template <int OW>
int summary_general(const void* offs, const uint8_t* vals, const uint8_t* validity, int64_t voff, int64_t n, int L,
                    const uint32_t* ids, int64_t n_clusters, int64_t max_len, uint32_t* n_reads,
                    uint32_t* n_distinct, int64_t* rep_row, hipStream_t s) {
    const int64_t nc1 = std::max<int64_t>(n_clusters, 1);
    ROGTK_HIP_CHECK(hipMemsetAsync(n_reads, 0, (size_t)nc1 * 4, s));
    ROGTK_HIP_CHECK(hipMemsetAsync(n_distinct, 0, (size_t)nc1 * 4, s));
    ROGTK_HIP_CHECK(hipMemsetAsync(rep_row, 0xFF, (size_t)nc1 * 8, s));
    if (n == 0) return ROGTK_OK;
    size_t sort_b = 0;
    ROGTK_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_b, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                       (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0, 64, s));
    Arena A;
    if (int rc = A.get(al(16) + al((size_t)nc1 * 8) + 3 * al((size_t)n * 8) + 3 * al((size_t)n * 4) + al(sort_b) + 256,
                       s))
        return rc;
    unsigned long long* cnt = A.take<unsigned long long>(2);
    unsigned long long* votes = A.take<unsigned long long>(nc1);
    int64_t* rows = A.take<int64_t>(n);
    uint64_t* key = A.take<uint64_t>(n);
    uint64_t* skey = A.take<uint64_t>(n);
    uint32_t* srank = A.take<uint32_t>(n);
    uint32_t* val = A.take<uint32_t>(n);
    uint32_t* sval = A.take<uint32_t>(n);
    void* tmp = A.take<uint8_t>((int64_t)sort_b);
    ROGTK_HIP_CHECK(hipMemsetAsync(cnt, 0, 16, s));
    ROGTK_HIP_CHECK(hipMemsetAsync(votes, 0, (size_t)nc1 * 8, s));
    hipLaunchKernelGGL(k_valid_rows, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, validity, voff, n, ids, n_clusters,
                       rows, cnt);
    ROGTK_HIP_CHECK(hipGetLastError());
    unsigned long long h[2];
    ROGTK_HIP_CHECK(hipMemcpyAsync(h, cnt, 16, hipMemcpyDeviceToHost, s));
    ROGTK_HIP_CHECK(hipStreamSynchronize(s));
    ROGTK_REQUIRE(h[1] == 0, ROGTK_E_INVALID, "cluster summary: a cluster id is >= n_clusters (%lld)",
                  (long long)n_clusters);
    const int64_t m = (int64_t)h[0];
    if (m == 0) return ROGTK_OK;
    // byte-lexicographic rank of every non-null row's string among the distinct strings
    int64_t n_strings = 0;
    if (int rc = irregular_cluster(offs, OW, vals, rows, m, max_len, nullptr, srank, &n_strings, s)) return rc;
    const dim3 g(grid_for(m, kBlock)), b(kBlock);
    hipLaunchKernelGGL(k_pair_keys, g, b, 0, s, rows, m, ids, srank, key, val);
    ROGTK_HIP_CHECK(hipGetLastError());
    size_t tb = sort_b;
    ROGTK_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, tb, key, skey, val, sval, (int)m, 0, 64, s));
    hipLaunchKernelGGL(k_vote_strings<OW>, dim3(tiles_for(m)), b, 0, s, offs, vals, skey, sval, m, L,
                       VoteTables{votes, n_reads, n_distinct});
    hipLaunchKernelGGL(k_pick_rows, g, b, 0, s, skey, sval, m, votes, rep_row);
    ROGTK_HIP_CHECK(hipGetLastError());
    return ROGTK_OK;
}

}  // namespace

int cluster_summary_set_method(int m) {
    ROGTK_REQUIRE(m == 0 || m == 1, ROGTK_E_INVALID, "summary method must be 0 (sort) or 1 (count table), got %d", m);
    g_summary_method.store(m);
    return ROGTK_OK;
}

int cluster_summary_packed_temp(int64_t n, int L, int64_t n_clusters, int64_t* bytes) {
    PackedLayout p;
    if (int rc = packed_layout(n, L, n_clusters, &p)) return rc;
    *bytes = (int64_t)p.total;
    return ROGTK_OK;
}

int launch_cluster_summary_packed(const uint32_t* codes, const uint64_t* regbits, int64_t n, int L,
                                  const uint32_t* ids, int64_t n_clusters, uint32_t* rep_code, uint32_t* n_reads,
                                  uint32_t* n_distinct, void* temp, int64_t temp_bytes, hipStream_t s) {
    PackedLayout p;
    if (int rc = packed_layout(n, L, n_clusters, &p)) return rc;
    ROGTK_REQUIRE((int64_t)p.total <= temp_bytes, ROGTK_E_INVALID, "temp_bytes %lld too small (need %lld)",
                  (long long)temp_bytes, (long long)p.total);
    uint8_t* t = (uint8_t*)temp;
    unsigned long long* cnt = (unsigned long long*)(t + p.off_cnt);
    unsigned long long* votes = (unsigned long long*)(t + p.off_votes);
    const uint32_t mask = L == 16 ? 0xFFFFFFFFu : (1u << (2 * L)) - 1u;
    if (n_clusters > 0) {
        ROGTK_HIP_CHECK(hipMemsetAsync(votes, 0, (size_t)n_clusters * 8, s));
        ROGTK_HIP_CHECK(hipMemsetAsync(n_reads, 0, (size_t)n_clusters * 4, s));
        ROGTK_HIP_CHECK(hipMemsetAsync(n_distinct, 0, (size_t)n_clusters * 4, s));
    }
    if (n > 0 && n_clusters > 0 && g_summary_method.load() == 1 && L <= kTableMaxLen) {
        const int64_t space = (int64_t)1 << (2 * L);
        uint32_t* tab = (uint32_t*)(t + p.off_tab);
        uint32_t* idtab = (uint32_t*)(t + p.off_idtab);
        ROGTK_HIP_CHECK(hipMemsetAsync(tab, 0, (size_t)space * 4, s));
        hipLaunchKernelGGL(k_table_count, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, codes, regbits, ids, n, mask,
                           tab, idtab);
        hipLaunchKernelGGL(k_table_vote, dim3(tiles_for(space)), dim3(kBlock), 0, s, tab, idtab, space, n_clusters,
                           VoteTables{votes, n_reads, n_distinct});
    } else if (n > 0 && n_clusters > 0) {
        const uint32_t* kin = codes;
        const uint32_t* vin = ids;
        if (regbits) {
            uint32_t* k0 = (uint32_t*)(t + p.off_key[0]);
            uint32_t* v0 = (uint32_t*)(t + p.off_val[0]);
            ROGTK_HIP_CHECK(hipMemsetAsync(cnt, 0, 16, s));
            hipLaunchKernelGGL(k_pack_regular, dim3(tiles_for(n)), dim3(kBlock), 0, s, codes, regbits, ids, n, mask,
                               k0, v0, cnt);
            ROGTK_HIP_CHECK(hipGetLastError());
            kin = k0;
            vin = v0;
        }
        uint32_t* k1 = (uint32_t*)(t + p.off_key[1]);
        uint32_t* v1 = (uint32_t*)(t + p.off_val[1]);
        size_t sb = p.sort_bytes;
        ROGTK_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(t + p.off_sort, sb, kin, k1, vin, v1, (int)n, 0, 2 * L, s));
        hipLaunchKernelGGL(k_vote_runs, dim3(tiles_for(n)), dim3(kBlock), 0, s, k1, v1, n,
                           regbits ? cnt : (const unsigned long long*)nullptr, mask, n_clusters,
                           VoteTables{votes, n_reads, n_distinct});
    }
    if (n_clusters > 0)
        hipLaunchKernelGGL(k_rep_codes, dim3(grid_for(n_clusters, kBlock)), dim3(kBlock), 0, s, votes, n_clusters,
                           rep_code);
    ROGTK_HIP_CHECK(hipGetLastError());
    return ROGTK_OK;
}

int launch_cluster_correct_packed(const uint32_t* ids, const uint64_t* regbits, int64_t n, const uint32_t* rep_code,
                                  int64_t n_clusters, uint32_t* out, hipStream_t s) {
    if (n <= 0) return ROGTK_OK;
    const uint32_t nc = (uint32_t)std::min<int64_t>(n_clusters, 0xFFFFFFFFll);
    const bool vec = (((uintptr_t)ids | (uintptr_t)out) & 15u) == 0;
    const int64_t n4 = vec ? n / 4 : 0;
    if (n4 > 0)
        hipLaunchKernelGGL(k_correct4, dim3(grid_for(n4, kBlock)), dim3(kBlock), 0, s, ids, regbits, n4, rep_code, nc,
                           out);
    if (4 * n4 < n)
        hipLaunchKernelGGL(k_correct1, dim3(grid_for(n - 4 * n4, kBlock)), dim3(kBlock), 0, s, ids, regbits, 4 * n4, n,
                           rep_code, nc, out);
    ROGTK_HIP_CHECK(hipGetLastError());
    return ROGTK_OK;
}

int cluster_summary_general(const DevCol& col, int L, const uint32_t* ids, int64_t n_clusters, int64_t max_len,
                            uint32_t* n_reads, uint32_t* n_distinct, int64_t* rep_row, hipStream_t s) {
    const auto [offsets, ow, values, validity, voff, n] = col;
    ROGTK_REQUIRE(n < (1ll << 31), ROGTK_E_UNSUPPORTED, "cluster summary: at most 2^31 - 1 rows");
    if (ow == 4)
        return summary_general<4>(offsets, values, validity, voff, n, L, ids, n_clusters, max_len, n_reads, n_distinct,
                                  rep_row, s);
    return summary_general<8>(offsets, values, validity, voff, n, L, ids, n_clusters, max_len, n_reads, n_distinct,
                              rep_row, s);
}

int representatives_temp(int64_t n_clusters, int64_t* bytes) {
    size_t tb = 0;
    ROGTK_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (const int64_t*)nullptr, (int64_t*)nullptr,
                                                     (int)(n_clusters + 1)));
    *bytes = (int64_t)(al((size_t)(n_clusters + 1) * 8) + al(tb));
    return ROGTK_OK;
}

int representatives_measure(const DevCol& col, const int64_t* rep_row, int64_t n_clusters, int64_t* out_offsets,
                            void* temp, int64_t temp_bytes, hipStream_t s) {
    const void* offsets = col.offsets;
    const int ow = col.ow;
    int64_t need = 0;
    if (int rc = representatives_temp(n_clusters, &need)) return rc;
    ROGTK_REQUIRE(temp && need <= temp_bytes, ROGTK_E_INVALID, "representatives: temp_bytes %lld too small (need %lld)",
                  (long long)temp_bytes, (long long)need);
    int64_t* lengths = (int64_t*)temp;
    const dim3 g(grid_for(n_clusters + 1, kBlock)), b(kBlock);
    if (ow == 4) hipLaunchKernelGGL(k_rep_lengths<4>, g, b, 0, s, offsets, rep_row, n_clusters, lengths);
    else hipLaunchKernelGGL(k_rep_lengths<8>, g, b, 0, s, offsets, rep_row, n_clusters, lengths);
    ROGTK_HIP_CHECK(hipGetLastError());
    const size_t head = al((size_t)(n_clusters + 1) * 8);
    size_t tb = (size_t)need - head;
    ROGTK_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum((uint8_t*)temp + head, tb, lengths, out_offsets,
                                                     (int)(n_clusters + 1), s));
    return ROGTK_OK;
}

int representatives_fill(const void* offsets, int ow, const uint8_t* values, const int64_t* rep_row, int64_t n_clusters,
                         const int64_t* out_offsets, uint8_t* out_values, hipStream_t s) {
    if (n_clusters <= 0) return ROGTK_OK;
    const dim3 g(grid_for(n_clusters, kBlock)), b(kBlock);
    if (ow == 4)
        hipLaunchKernelGGL(k_rep_fill<4>, g, b, 0, s, offsets, values, rep_row, n_clusters, out_offsets, out_values);
    else
        hipLaunchKernelGGL(k_rep_fill<8>, g, b, 0, s, offsets, values, rep_row, n_clusters, out_offsets, out_values);
    ROGTK_HIP_CHECK(hipGetLastError());
    return ROGTK_OK;
}

int corrected_fill(const DevCol& col, const uint32_t* ids, int64_t n_clusters, const int64_t* rep_row,
                   uint8_t* out_values, hipStream_t s) {
    const auto [offsets, ow, values, validity, voff, n] = col;
    if (n <= 0) return ROGTK_OK;
    const dim3 g(grid_for(n, kBlock)), b(kBlock);
    if (ow == 4)
        hipLaunchKernelGGL(k_corrected_fill<4>, g, b, 0, s, offsets, values, validity, voff, n, ids, n_clusters,
                           rep_row, out_values);
    else
        hipLaunchKernelGGL(k_corrected_fill<8>, g, b, 0, s, offsets, values, validity, voff, n, ids, n_clusters,
                           rep_row, out_values);
    ROGTK_HIP_CHECK(hipGetLastError());
    return ROGTK_OK;
}

}  // namespace rogtk
