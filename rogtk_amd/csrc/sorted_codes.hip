// sorted_codes.hip — the front end of the sort engines (long_cluster.hip, directional.hip;
// DESIGN.md §4): a device string column -> the sorted distinct 2-bit codes of its regular rows.
//
//   pack     every row is classified (null / regular / irregular). The regular rows' (code,
//            row) pairs are appended to key / row and the irregular rows to irr, in any order
//            (both are sorted later); null rows get cluster id 0xFFFFFFFF. A workgroup
//            classifies kPackTile rows and reserves its two ranges with one atomic each.
//   sort     radix sort of the pairs over the 2 L code bits (u32 keys for L <= 16, u64 above;
//            u32 row payloads: n < 2^31).
//   groups    with one u32 key per row the pack kernel builds the u64 composite
//            key << 2 L | code and records the largest key of the regular and of the irregular
//            rows; the sort then runs over exactly 2 L + bit_width(largest key) bits and D
//            holds composites. A template parameter: the ungrouped kernels are unchanged.
//   distinct flag every sorted row whose code differs from its predecessor's; the inclusive
//            scan of the flags is the row's index into the distinct codes D, and the heads of
//            the runs write D (and, when counts are wanted, their positions: C[j] is the
//            distance to the next head).
//
// Two stream-ordered allocations: the row-sized arrays, and after m is known D and C together
// with whatever per-code scratch the calling engine asks for (ExtraCodeBytes, rogtk_internal.h).
#include <hipcub/hipcub.hpp>

#include "column_util.h"
#include "level2.h"

namespace rogtk {
namespace {

constexpr int kBlock = 256;
constexpr int kPackRows = 4;  // rows per thread of k_pack
constexpr int kPackTile = kBlock * kPackRows;

// cnt[0] regular rows, cnt[1] irregular rows, cnt[2] the longest irregular row; GROUPED: the
// two u32 halves of cnt[3] are the largest key of a regular and of an irregular row
template <int OW, class K, bool GROUPED>
__global__ void __launch_bounds__(kBlock)
k_pack(const void* __restrict__ offs, const uint8_t* __restrict__ vals, const uint8_t* __restrict__ validity,
       int64_t voff, int64_t n, int L, K* __restrict__ key, uint32_t* __restrict__ row, int64_t* __restrict__ irr,
       uint32_t* __restrict__ cluster_id, unsigned long long* __restrict__ cnt,
       const uint32_t* __restrict__ groups) {
    constexpr int kWaves = kBlock / 64;
    __shared__ uint32_t pre_r[kPackRows * kWaves], pre_i[kPackRows * kWaves];
    [[maybe_unused]] __shared__ uint32_t gmax[2 * kWaves];
    [[maybe_unused]] uint32_t gmax_r = 0, gmax_i = 0;
    __shared__ unsigned long long base[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile = (int64_t)blockIdx.x * kPackTile;
    uint64_t code[kPackRows], rmask[kPackRows], imask[kPackRows];
    unsigned long long longest = 0;
    for (int r = 0; r < kPackRows; ++r) {
        const int64_t i = tile + (int64_t)r * kBlock + threadIdx.x;
        bool valid = false, regular = false;
        uint64_t c = 0;
        if (i < n) {
            valid = row_valid(validity, voff, i);
            if (valid) {
                int64_t st, len;
                span<OW>(offs, i, st, len);
                regular = L >= 1 && L <= 32 && len == L;
                for (int j = 0; regular && j < L; ++j) {
                    const int b = base_code(vals[st + j]);
                    regular = b >= 0;
                    c = (c << 2) | (uint64_t)(b & 3);
                }
                if (!regular) longest = max(longest, (unsigned long long)len);
                if constexpr (GROUPED) {
                    const uint32_t g = groups[i];
                    if (regular) {
                        gmax_r = max(gmax_r, g);
                        if (L < 32) c |= (uint64_t)g << (2 * L);  // L == 32: only key 0 fits (checked on the host)
                    } else {
                        gmax_i = max(gmax_i, g);
                    }
                }
            } else {
                cluster_id[i] = 0xFFFFFFFFu;
            }
        }
        code[r] = c;
        rmask[r] = __ballot(regular);
        imask[r] = __ballot(valid && !regular);
        if (lane == 0) {
            pre_r[r * kWaves + wave] = (uint32_t)__popcll(rmask[r]);
            pre_i[r * kWaves + wave] = (uint32_t)__popcll(imask[r]);
        }
    }
    for (int d = 32; d; d >>= 1) longest = max(longest, (unsigned long long)__shfl_xor(longest, d));
    if (lane == 0 && longest) atomicMax(&cnt[2], longest);
    if constexpr (GROUPED) {
        for (int d = 32; d; d >>= 1) {
            gmax_r = max(gmax_r, (uint32_t)__shfl_xor(gmax_r, d));
            gmax_i = max(gmax_i, (uint32_t)__shfl_xor(gmax_i, d));
        }
        if (lane == 0) {
            gmax[wave] = gmax_r;
            gmax[kWaves + wave] = gmax_i;
        }
    }
    __syncthreads();
    if constexpr (GROUPED) {
        if (threadIdx.x < 2) {  // one atomic per workgroup and kind
            uint32_t g = 0;
            for (int w = 0; w < kWaves; ++w) g = max(g, gmax[threadIdx.x * kWaves + w]);
            if (g) atomicMax((uint32_t*)(cnt + 3) + threadIdx.x, g);
        }
    }
    if (threadIdx.x == 0) {
        uint32_t sr = 0, si = 0;
        for (int k = 0; k < kPackRows * kWaves; ++k) {
            const uint32_t cr = pre_r[k], ci = pre_i[k];
            pre_r[k] = sr;
            pre_i[k] = si;
            sr += cr;
            si += ci;
        }
        base[0] = sr ? atomicAdd(&cnt[0], (unsigned long long)sr) : 0ull;
        base[1] = si ? atomicAdd(&cnt[1], (unsigned long long)si) : 0ull;
    }
    __syncthreads();
    const uint64_t below = (1ull << lane) - 1ull;
    for (int r = 0; r < kPackRows; ++r) {
        const int64_t i = tile + (int64_t)r * kBlock + threadIdx.x;
        if ((rmask[r] >> lane) & 1ull) {
            const int64_t p = (int64_t)base[0] + pre_r[r * kWaves + wave] + __popcll(rmask[r] & below);
            key[p] = (K)code[r];
            row[p] = (uint32_t)i;
        } else if ((imask[r] >> lane) & 1ull) {
            irr[(int64_t)base[1] + pre_i[r * kWaves + wave] + __popcll(imask[r] & below)] = i;
        }
    }
}

// 1 where a sorted row's code differs from its predecessor's (row 0: 0), so that the
// inclusive scan is the row's index into the distinct codes
template <class K>
__global__ void k_steps(const K* __restrict__ key, int64_t n, uint32_t* __restrict__ flag) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n) return;
    flag[k] = k > 0 && key[k - 1] != key[k];
}

template <class K>
__global__ void k_distinct(const K* __restrict__ key, const uint32_t* __restrict__ flag,
                           const uint32_t* __restrict__ idx, int64_t n, uint64_t* __restrict__ D,
                           uint32_t* __restrict__ head) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n || (k > 0 && !flag[k])) return;
    D[idx[k]] = (uint64_t)key[k];
    if (head) head[idx[k]] = (uint32_t)k;
}

__global__ void k_counts(const uint32_t* __restrict__ head, int64_t m, int64_t n, uint32_t* __restrict__ C) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    C[j] = (j + 1 < m ? head[j + 1] : (uint32_t)n) - head[j];
}

template <int OW, class K, bool GROUPED>
int run(const void* offs, const uint8_t* vals, const uint8_t* validity, int64_t voff, int64_t n, int L,
        bool want_counts, const ExtraCodeBytes* extra, uint32_t* cluster_id, SortedCodes* out, hipStream_t s,
        const uint32_t* groups) {
    const dim3 b(kBlock);
    int bits = L >= 1 && L <= 32 ? 2 * L : 2;  // any other L: no row is regular
    size_t sort_b = 0, scan_b = 0;
    // (sized for the widest key the grouped sort can run over)
    ROGTK_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_b, (const K*)nullptr, (K*)nullptr,
                                                       (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0,
                                                       GROUPED ? 64 : bits, s));
    ROGTK_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, scan_b, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                     (int)n, s));
    const size_t tmp_b = std::max(sort_b, scan_b);
    Arena& A = out->rows_mem;
    if (int rc = A.get(al(64) + 2 * al((size_t)n * sizeof(K)) + 4 * al((size_t)n * 4) + al((size_t)n * 8) + al(tmp_b),
                       s))
        return rc;
    unsigned long long* cnt = A.take<unsigned long long>(8);
    K* key = A.take<K>(n);
    K* skey = A.take<K>(n);
    uint32_t* row = A.take<uint32_t>(n);
    uint32_t* srow = A.take<uint32_t>(n);
    uint32_t* flag = A.take<uint32_t>(n);
    uint32_t* idx = A.take<uint32_t>(n);
    int64_t* irr = A.take<int64_t>(n);
    void* tmp = A.take<uint8_t>((int64_t)tmp_b);
    ROGTK_HIP_CHECK(hipMemsetAsync(cnt, 0, 64, s));
    hipLaunchKernelGGL((k_pack<OW, K, GROUPED>), dim3(grid_for(n, kPackTile)), b, 0, s, offs, vals, validity, voff, n,
                       L, key, row, irr, cluster_id, cnt, groups);
    ROGTK_HIP_CHECK(hipGetLastError());
    unsigned long long h[4];
    ROGTK_HIP_CHECK(hipMemcpyAsync(h, cnt, 32, hipMemcpyDeviceToHost, s));
    ROGTK_HIP_CHECK(hipStreamSynchronize(s));
    if (GROUPED) {
        out->max_group = (uint32_t)h[3];
        out->max_irr_group = (uint32_t)(h[3] >> 32);
        int gb = 0;
        while (gb < 32 && (out->max_group >> gb)) ++gb;
        ROGTK_REQUIRE(h[0] == 0 || bits + gb <= 64, ROGTK_E_UNSUPPORTED,
                      "grouped: umi_len %d with a group key of %d bits needs a %d-bit sort key (at most 64)", L, gb,
                      bits + gb);
        bits += gb;
    }
    out->key_bits = bits;
    const int64_t n_reg = (int64_t)h[0];
    out->n_reg = n_reg;
    out->n_irr = (int64_t)h[1];
    out->max_irr_len = (int64_t)h[2];
    out->irr = irr;
    out->spare = (int64_t*)(cnt + 4);
    if (n_reg == 0) return ROGTK_OK;
    const dim3 g(grid_for(n_reg, kBlock));
    size_t tb = tmp_b;
    ROGTK_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, tb, key, skey, row, srow, (int)n_reg, 0, bits, s));
    hipLaunchKernelGGL(k_steps<K>, g, b, 0, s, skey, n_reg, flag);
    tb = tmp_b;
    ROGTK_HIP_CHECK(hipcub::DeviceScan::InclusiveSum(tmp, tb, flag, idx, (int)n_reg, s));
    uint32_t last = 0;
    ROGTK_HIP_CHECK(hipMemcpyAsync(&last, idx + n_reg - 1, 4, hipMemcpyDeviceToHost, s));
    ROGTK_HIP_CHECK(hipStreamSynchronize(s));
    const int64_t m = (int64_t)last + 1;
    size_t extra_b = 0;
    if (extra)
        if (int rc = (*extra)(m, &extra_b)) return rc;
    Arena& B = out->codes_mem;
    if (int rc = B.get(al((size_t)m * 8) + (want_counts ? 2 * al((size_t)m * 4) : 0) + extra_b, s)) return rc;
    uint64_t* D = B.take<uint64_t>(m);
    uint32_t* C = want_counts ? B.take<uint32_t>(m) : nullptr;
    uint32_t* head = want_counts ? B.take<uint32_t>(m) : nullptr;  // scratch of k_counts
    hipLaunchKernelGGL(k_distinct<K>, g, b, 0, s, skey, flag, idx, n_reg, D, head);
    if (want_counts) hipLaunchKernelGGL(k_counts, dim3(grid_for(m, kBlock)), b, 0, s, head, m, n_reg, C);
    ROGTK_HIP_CHECK(hipGetLastError());
    out->m = m;
    out->row = srow;
    out->idx = idx;
    out->D = D;
    out->C = C;
    return ROGTK_OK;
}

}  // namespace

int sorted_distinct_codes(const DevCol& col, int L, bool want_counts, const ExtraCodeBytes* extra, uint32_t* cluster_id,
                          SortedCodes* out, hipStream_t s, const uint32_t* groups) {
    const int ow = col.ow;
    const int64_t n = col.n;
    ROGTK_REQUIRE(n > 0 && n < (1ll << 31), ROGTK_E_UNSUPPORTED, "sorted codes: n %lld outside 1..2^31-1",
                  (long long)n);
    auto go = [&](auto ow_tag, auto key_tag, auto grouped_tag) {
        return run<decltype(ow_tag)::value, decltype(key_tag), decltype(grouped_tag)::value>(
            col.offsets, col.values, col.validity, col.voff, n, L, want_counts, extra, cluster_id, out, s, groups);
    };
    using W4 = std::integral_constant<int, 4>;
    using W8 = std::integral_constant<int, 8>;
    if (groups)  // composites are u64 whatever L
        return ow == 4 ? go(W4{}, uint64_t{}, std::true_type{}) : go(W8{}, uint64_t{}, std::true_type{});
    const bool wide = L > 16;
    if (ow == 4) return wide ? go(W4{}, uint64_t{}, std::false_type{}) : go(W4{}, uint32_t{}, std::false_type{});
    return wide ? go(W8{}, uint64_t{}, std::false_type{}) : go(W8{}, uint32_t{}, std::false_type{});
}

}  // namespace rogtk
