// barcode.hip — cell-barcode correction against a whitelist.
//
//   handle   the whitelist as 2-bit codes (u64, first base in the highest digit), radix-sorted
//            with the caller's row as payload; adjacent equal codes are refused. On the device
//            stay the sorted codes, the permutation back to the caller's order, the codes in
//            the caller's order (the corrected strings are unpacked from them) and a
//            direct-address table start[4^P + 1] over the top P digits: a lookup is two
//            adjacent table loads and a binary search inside one bucket.
//   exact    k_bc_exact, one pass over the rows (4 rows per lane, ballots, one atomic per
//            workgroup and list, as k_pack of sorted_codes.hip): classify and pack every row,
//            look the rows without an unknown position up, write index / status of the null,
//            exact and candidate-less rows, add to exact_counts (through an LDS count table per
//            workgroup, flushed once) and append the rows that need a neighbour search to the
//            miss list.
//   probe    k_bc_probe over the miss list, a kernel of its own because under
//            ambiguous="counts" it reads the finished exact_counts. The 3 L (or 4) lookups of
//            one miss are run by one lane (kBarcodeProbeLane, the default: the faster of the
//            two as measured), or spread over the lanes of a wave and reduced there
//            (kBarcodeProbeWave); the answers are identical.
//   strings  the corrected column of the host entry: offsets are the scan of
//            status <= 1 ? L : 0, the bytes are unpacked from the whitelist code.
//
// Plain HIP, no device-wide synchronisation inside a kernel, stream-ordered scratch per call.
#include <hipcub/hipcub.hpp>

#include <atomic>

#include "column_util.h"
#include "level2.h"

namespace rogtk {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kRows = 4;  // rows per thread of k_bc_exact
constexpr int kTile = kBlock * kRows;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint8_t kNoUnknown = 0xFF;
constexpr int kCountBits = 11;  // the exact pass's LDS count table: 2048 (entry, rows) slots
constexpr int kCountSlots = 1 << kCountBits;
constexpr int kExactBlocks = 2048;  // its grid: 8 workgroups per CU
constexpr int kMaxPrefixDigits = 12;  // start[] is at most (4^12 + 1) * 4 B = 64 MiB

std::atomic<int> g_probe{kBarcodeProbeLane};  // the faster at both measured W

struct Whitelist {
    int device = -1;
    int64_t W = 0;
    int L = 0, P = 0;
    int64_t bytes = 0;
    uint8_t* mem = nullptr;
    const uint64_t* sorted = nullptr;  // [W] codes ascending
    const uint32_t* perm = nullptr;    // [W] caller's row of sorted[k]
    const uint32_t* start = nullptr;   // [4^P + 1] first sorted entry of every P-digit prefix
    const uint64_t* by_row = nullptr;  // [W] codes in the caller's order
};

// what the kernels take by value
struct View {
    const uint64_t* sorted;
    const uint32_t* perm;
    const uint32_t* start;
    uint32_t W;
    int L, shift;  // shift = 2 (L - P): code >> shift is the prefix
    int plain;     // 1: binary search over the whole array (measurements only)
};

// the sorted position of code c, or kNone
__device__ __forceinline__ uint32_t find(const View& v, uint64_t c) {
    uint32_t lo = 0, hi = v.W;
    if (!v.plain) {
        const uint64_t p = c >> v.shift;
        lo = v.start[p];
        hi = v.start[p + 1];
    }
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint64_t x = v.sorted[mid];
        if (x == c) return mid;
        if (x < c) lo = mid + 1;
        else hi = mid;
    }
    return kNone;
}

// table[w] += 1 for every lane with `has`, equal w of a wave combined into one atomic for the
// first few distinct values (a large cell owns many nearby rows); called by whole waves
__device__ __forceinline__ void wave_add(uint32_t* __restrict__ table, bool has, uint32_t w, int lane) {
    uint64_t todo = __ballot(has);
    for (int round = 0; round < 4 && todo; ++round) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t lw = (uint32_t)__shfl((int)w, leader);
        const uint64_t same = __ballot(has && w == lw) & todo;
        if (lane == leader) atomicAdd(&table[lw], (uint32_t)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) atomicAdd(&table[w], 1u);
}

// thread p: the first sorted entry whose prefix is >= p (p = 4^P: W)
__global__ void k_bc_start(const uint64_t* __restrict__ sorted, uint32_t W, int shift, int64_t entries,
                           uint32_t* __restrict__ start) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= entries) return;
    uint32_t lo = 0, hi = W;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)(sorted[mid] >> shift) < p) lo = mid + 1;
        else hi = mid;
    }
    start[p] = lo;
}

// the smallest caller's row whose code equals that of an earlier row (the sort is stable)
__global__ void k_bc_dup(const uint64_t* __restrict__ sorted, const uint32_t* __restrict__ perm, int64_t W,
                         uint32_t* __restrict__ first_dup) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k < 1 || k >= W) return;
    if (sorted[k] == sorted[k - 1]) atomicMin(first_dup, perm[k]);
}

__global__ void k_bc_iota(uint32_t* __restrict__ a, int64_t n) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k < n) a[k] = (uint32_t)k;
}

// exact_counts[w] += 1 through the workgroup's LDS table (open addressing, a few probes); a
// full neighbourhood falls through to the global atomic
__device__ __forceinline__ void lds_count(uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                          uint32_t* __restrict__ exact_counts, uint32_t w) {
    const uint32_t h = (w * 2654435761u) >> (32 - kCountBits);
    for (int k = 0; k < 8; ++k) {
        const uint32_t slot = (h + (uint32_t)k) & (kCountSlots - 1);
        const uint32_t old = atomicCAS(&keys[slot], kNone, w);
        if (old == kNone || old == w) {
            atomicAdd(&vals[slot], 1u);
            return;
        }
    }
    atomicAdd(&exact_counts[w], 1u);
}

// cnt[0] misses; cnt[1..5] rows of status 0..4. A workgroup walks tiles of kTile rows
// (grid-stride) and keeps its exact rows' counts in LDS until the end: a large cell's rows then
// cost one global atomic per workgroup and not one each, all on one address.
template <int OW>
__global__ void __launch_bounds__(kBlock)
k_bc_exact(const void* __restrict__ offs, const uint8_t* __restrict__ vals, const uint8_t* __restrict__ validity,
           int64_t voff, int64_t n, View v, uint32_t* __restrict__ index, uint8_t* __restrict__ status,
           uint32_t* __restrict__ exact_counts, uint64_t* __restrict__ miss_code, uint32_t* __restrict__ miss_row,
           uint8_t* __restrict__ miss_unk, unsigned long long* __restrict__ cnt) {
    __shared__ uint32_t ckey[kCountSlots], cval[kCountSlots];
    __shared__ uint32_t pre_m[kRows * kWaves];
    __shared__ uint32_t tot[3 * kWaves];  // exact, candidate-less, null rows of every wave
    __shared__ unsigned long long base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool write = index != nullptr;  // false: count only
    const uint64_t below = (1ull << lane) - 1ull;
    for (int k = threadIdx.x; k < kCountSlots; k += kBlock) {
        ckey[k] = kNone;
        cval[k] = 0;
    }
    __syncthreads();
    uint32_t n_exact = 0, n_none = 0, n_null = 0;
    const int64_t n_tiles = (n + kTile - 1) / kTile;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t tile = t * kTile;
        uint64_t code[kRows], mmask[kRows];
        uint8_t unk[kRows];
        for (int r = 0; r < kRows; ++r) {
            const int64_t i = tile + (int64_t)r * kBlock + threadIdx.x;
            bool is_null = false, none = false, exact = false, miss = false;
            uint64_t c = 0;
            uint32_t w = 0;
            int u = kNoUnknown;
            if (i < n) {
                if (!row_valid(validity, voff, i)) {
                    is_null = true;
                } else {
                    int64_t st, len;
                    span<OW>(offs, i, st, len);
                    int n_unk = 0;
                    if (len != v.L) n_unk = 2;
                    for (int j = 0; n_unk < 2 && j < v.L; ++j) {
                        int b = base_code(vals[st + j]);
                        if (b < 0) {
                            ++n_unk;
                            u = j;
                            b = 0;
                        }
                        c = (c << 2) | (uint64_t)b;
                    }
                    if (n_unk >= 2) {
                        none = true;
                    } else if (n_unk == 1) {
                        miss = true;
                    } else {
                        const uint32_t e = find(v, c);
                        if (e != kNone) {
                            exact = true;
                            w = v.perm[e];
                            lds_count(ckey, cval, exact_counts, w);
                        } else {
                            miss = true;
                        }
                    }
                }
                if (write && !miss) {
                    index[i] = exact ? w : kNone;
                    status[i] = exact ? ROGTK_BC_EXACT : none ? ROGTK_BC_NO_MATCH : ROGTK_BC_NULL;
                }
            }
            code[r] = c;
            unk[r] = (uint8_t)u;
            mmask[r] = __ballot(miss);
            n_exact += (uint32_t)__popcll(__ballot(exact));
            n_none += (uint32_t)__popcll(__ballot(none));
            n_null += (uint32_t)__popcll(__ballot(is_null));
            if (lane == 0) pre_m[r * kWaves + wave] = (uint32_t)__popcll(mmask[r]);
        }
        if (!write) continue;
        __syncthreads();
        if (threadIdx.x == 0) {  // one atomic per tile for the miss list
            uint32_t sm = 0;
            for (int k = 0; k < kRows * kWaves; ++k) {
                const uint32_t cm = pre_m[k];
                pre_m[k] = sm;
                sm += cm;
            }
            base = sm ? atomicAdd(&cnt[0], (unsigned long long)sm) : 0ull;
        }
        __syncthreads();
        for (int r = 0; r < kRows; ++r) {
            if (!((mmask[r] >> lane) & 1ull)) continue;
            const int64_t i = tile + (int64_t)r * kBlock + threadIdx.x;
            const int64_t p = (int64_t)base + pre_m[r * kWaves + wave] + __popcll(mmask[r] & below);
            miss_code[p] = code[r];
            miss_row[p] = (uint32_t)i;
            miss_unk[p] = unk[r];
        }
        __syncthreads();  // pre_m and base are rewritten by the next tile
    }
    if (lane == 0) {
        tot[wave] = n_exact;
        tot[kWaves + wave] = n_none;
        tot[2 * kWaves + wave] = n_null;
    }
    __syncthreads();
    if (threadIdx.x < 3) {  // one atomic per workgroup and total
        uint32_t sum = 0;
        for (int k = 0; k < kWaves; ++k) sum += tot[threadIdx.x * kWaves + k];
        const int slot = threadIdx.x == 0   ? 1 + ROGTK_BC_EXACT
                         : threadIdx.x == 1 ? 1 + ROGTK_BC_NO_MATCH
                                            : 1 + ROGTK_BC_NULL;
        if (sum) atomicAdd(&cnt[slot], (unsigned long long)sum);
    }
    for (int k = threadIdx.x; k < kCountSlots; k += kBlock)
        if (cval[k]) atomicAdd(&exact_counts[ckey[k]], cval[k]);
}

// the candidates of one miss seen so far: how many, the largest prior count among them, the
// whitelist row that has it, and whether a second candidate has it too
struct Cand {
    uint32_t n, best, entry, tied;
};

__device__ __forceinline__ Cand merge(const Cand& a, const Cand& b) {
    if (a.n == 0) return b;
    if (b.n == 0) return a;
    Cand r;
    r.n = a.n + b.n;
    if (a.best > b.best) {
        r.best = a.best, r.entry = a.entry, r.tied = a.tied;
    } else if (b.best > a.best) {
        r.best = b.best, r.entry = b.entry, r.tied = b.tied;
    } else {
        r.best = a.best, r.entry = min(a.entry, b.entry), r.tied = 1;
    }
    return r;
}

// lookup j of a miss: the code with digit pos replaced (no unknown: j / 3 is the position from
// the first base, j % 3 the substitute; one unknown: j is the base at that position)
__device__ __forceinline__ void probe(const View& v, uint64_t c, int u, int j, const uint32_t* __restrict__ prior,
                                      Cand& acc) {
    uint64_t q;
    if (u == kNoUnknown) {
        const int sh = 2 * (v.L - 1 - j / 3);
        const uint64_t orig = (c >> sh) & 3ull;
        const uint64_t nb = (orig + 1 + (uint64_t)(j % 3)) & 3ull;
        q = c ^ ((orig ^ nb) << sh);
    } else {
        q = c | ((uint64_t)j << (2 * (v.L - 1 - u)));
    }
    const uint32_t e = find(v, q);
    if (e == kNone) return;
    const uint32_t w = v.perm[e];
    acc = merge(acc, Cand{1u, prior ? prior[w] : 0u, w, 0u});
}

// 0 corrected (entry), 1 ambiguous, 2 no_match
__device__ __forceinline__ int resolve(const Cand& a, int reject) {
    if (a.n == 0) return 2;
    if (a.n == 1) return 0;
    return reject || a.tied ? 1 : 0;
}

// LANE = false: a wave per miss, the lookups over its lanes; true: a lane per miss.
// prior: the caller's counts or this call's exact_counts (NULL under reject)
template <bool LANE>
__global__ void __launch_bounds__(kBlock)
k_bc_probe(const uint64_t* __restrict__ miss_code, const uint32_t* __restrict__ miss_row,
           const uint8_t* __restrict__ miss_unk, int64_t n_miss, View v, const uint32_t* __restrict__ prior,
           int reject, uint32_t* __restrict__ index, uint8_t* __restrict__ status, uint32_t* __restrict__ counts,
           unsigned long long* __restrict__ cnt) {
    __shared__ uint32_t tot[3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 3) tot[threadIdx.x] = 0;
    __syncthreads();
    const int64_t m = LANE ? (int64_t)blockIdx.x * kBlock + threadIdx.x : (int64_t)blockIdx.x * kWaves + wave;
    const bool live = m < n_miss;
    Cand acc{0u, 0u, 0u, 0u};
    if (live) {
        const uint64_t c = miss_code[m];
        const int u = miss_unk[m];
        const int np = u == kNoUnknown ? 3 * v.L : 4;
        if (LANE) {
            for (int j = 0; j < np; ++j) probe(v, c, u, j, prior, acc);
        } else {
            for (int j = lane; j < np; j += 64) probe(v, c, u, j, prior, acc);
        }
    }
    if (!LANE) {
        for (int d = 32; d; d >>= 1) {
            Cand o;
            o.n = (uint32_t)__shfl_xor((int)acc.n, d);
            o.best = (uint32_t)__shfl_xor((int)acc.best, d);
            o.entry = (uint32_t)__shfl_xor((int)acc.entry, d);
            o.tied = (uint32_t)__shfl_xor((int)acc.tied, d);
            acc = merge(acc, o);
        }
    }
    const int kind = resolve(acc, reject);
    const bool writer = live && (LANE || lane == 0);
    if (writer) {
        const uint32_t row = miss_row[m];
        index[row] = kind == 0 ? acc.entry : kNone;
        status[row] = kind == 0 ? ROGTK_BC_CORRECTED : kind == 1 ? ROGTK_BC_AMBIGUOUS : ROGTK_BC_NO_MATCH;
    }
    if (LANE) {
        if (counts) wave_add(counts, writer && kind == 0, acc.entry, lane);
        for (int k = 0; k < 3; ++k) {
            const uint64_t b = __ballot(writer && kind == k);
            if (lane == 0 && b) atomicAdd(&tot[k], (uint32_t)__popcll(b));
        }
    } else if (writer) {
        if (counts && kind == 0) atomicAdd(&counts[acc.entry], 1u);
        atomicAdd(&tot[kind], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 3 && tot[threadIdx.x]) {
        const int slot = threadIdx.x == 0   ? 1 + ROGTK_BC_CORRECTED
                         : threadIdx.x == 1 ? 1 + ROGTK_BC_AMBIGUOUS
                                            : 1 + ROGTK_BC_NO_MATCH;
        atomicAdd(&cnt[slot], (unsigned long long)tot[threadIdx.x]);
    }
}

__global__ void k_bc_lengths(const uint8_t* __restrict__ status, int64_t n, int L, int64_t* __restrict__ len) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    len[i] = i < n && status[i] <= ROGTK_BC_CORRECTED ? L : 0;
}

__global__ void k_bc_fill(const uint32_t* __restrict__ index, const uint8_t* __restrict__ status, int64_t n, int L,
                          const uint64_t* __restrict__ by_row, const int64_t* __restrict__ out_offsets,
                          uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || status[i] > ROGTK_BC_CORRECTED) return;
    const uint64_t c = by_row[index[i]];
    uint8_t* o = out + out_offsets[i];
    for (int j = 0; j < L; ++j) o[j] = (uint8_t)"ACGT"[(c >> (2 * (L - 1 - j))) & 3ull];
}

int prefix_digits(int64_t W, int L) {
    int p = 1;
    while (p < L && p < kMaxPrefixDigits && (1ll << (2 * p)) < W) ++p;  // about log4 W
    return p;
}

View view_of(const Whitelist* w) {
    const int probe = g_probe.load(std::memory_order_relaxed);
    return View{w->sorted, w->perm, w->start, (uint32_t)w->W, w->L, 2 * (w->L - w->P), (probe & kBarcodePlainSearch) ? 1 : 0};
}

int check_device(const Whitelist* w) {
    int dev = -1;
    ROGTK_HIP_CHECK(hipGetDevice(&dev));
    ROGTK_REQUIRE(dev == w->device, ROGTK_E_INVALID, "barcode whitelist: built on device %d, the current device is %d",
                  w->device, dev);
    return ROGTK_OK;
}

}  // namespace

int barcode_set_probe(int probe) {
    ROGTK_REQUIRE(probe >= 0 && probe <= (kBarcodeProbeLane | kBarcodePlainSearch), ROGTK_E_INVALID,
                  "barcode probe %d: 0 wave per miss, 1 lane per miss, +2 without the prefix table", probe);
    g_probe.store(probe, std::memory_order_relaxed);
    return ROGTK_OK;
}

void barcode_whitelist_free(void* handle) {
    Whitelist* w = (Whitelist*)handle;
    if (!w) return;
    if (w->mem) (void)hipFree(w->mem);
    delete w;
}

int barcode_whitelist_info(const void* handle, int64_t* W, int* L, int* prefix, int64_t* device_bytes) {
    const Whitelist* w = (const Whitelist*)handle;
    ROGTK_REQUIRE(w, ROGTK_E_INVALID, "barcode whitelist: NULL handle");
    if (W) *W = w->W;
    if (L) *L = w->L;
    if (prefix) *prefix = w->P;
    if (device_bytes) *device_bytes = w->bytes;
    return ROGTK_OK;
}

int barcode_whitelist_build(const uint64_t* host_codes, int64_t W, int L, void** out, hipStream_t s) {
    ROGTK_REQUIRE(W >= 1 && W < (1ll << 32) - 1 && L >= 1 && L <= 32, ROGTK_E_INVALID,
                  "barcode whitelist: W %lld, L %d", (long long)W, L);
    Whitelist* w = new Whitelist();
    auto run = [&]() -> int {
        ROGTK_HIP_CHECK(hipGetDevice(&w->device));
        w->W = W;
        w->L = L;
        w->P = prefix_digits(W, L);
        const int64_t entries = (1ll << (2 * w->P)) + 1;
        w->bytes = (int64_t)(2 * al((size_t)W * 8) + al((size_t)W * 4) + al((size_t)entries * 4));
        ROGTK_HIP_CHECK(hipMalloc((void**)&w->mem, (size_t)w->bytes));
        uint8_t* p = w->mem;
        uint64_t* sorted = (uint64_t*)p;
        p += al((size_t)W * 8);
        uint64_t* by_row = (uint64_t*)p;
        p += al((size_t)W * 8);
        uint32_t* perm = (uint32_t*)p;
        p += al((size_t)W * 4);
        uint32_t* start = (uint32_t*)p;
        size_t sort_b = 0;
        ROGTK_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_b, (const uint64_t*)nullptr,
                                                           (uint64_t*)nullptr, (const uint32_t*)nullptr,
                                                           (uint32_t*)nullptr, W, 0, 2 * L, s));
        Arena A;
        if (int rc = A.get(al(64) + al((size_t)W * 4) + al(sort_b), s)) return rc;
        uint32_t* first_dup = A.take<uint32_t>(16);
        uint32_t* iota = A.take<uint32_t>(W);
        void* tmp = A.take<uint8_t>((int64_t)sort_b);
        ROGTK_HIP_CHECK(hipMemcpyAsync(by_row, host_codes, (size_t)W * 8, hipMemcpyHostToDevice, s));
        ROGTK_HIP_CHECK(hipMemsetAsync(first_dup, 0xFF, 64, s));
        const dim3 b(kBlock), g(grid_for(W, kBlock));
        hipLaunchKernelGGL(k_bc_iota, g, b, 0, s, iota, W);
        ROGTK_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, sort_b, (const uint64_t*)by_row, sorted,
                                                           (const uint32_t*)iota, perm, W, 0, 2 * L, s));
        hipLaunchKernelGGL(k_bc_dup, g, b, 0, s, (const uint64_t*)sorted, (const uint32_t*)perm, W, first_dup);
        hipLaunchKernelGGL(k_bc_start, dim3(grid_for(entries, kBlock)), b, 0, s, (const uint64_t*)sorted, (uint32_t)W,
                           2 * (L - w->P), entries, start);
        ROGTK_HIP_CHECK(hipGetLastError());
        uint32_t dup = kNone;
        ROGTK_HIP_CHECK(hipMemcpyAsync(&dup, first_dup, 4, hipMemcpyDeviceToHost, s));
        ROGTK_HIP_CHECK(hipStreamSynchronize(s));
        ROGTK_REQUIRE(dup == kNone, ROGTK_E_INVALID, "barcode whitelist: row %u repeats an earlier barcode", dup);
        w->sorted = sorted;
        w->by_row = by_row;
        w->perm = perm;
        w->start = start;
        return ROGTK_OK;
    };
    const int rc = run();
    if (rc) {
        barcode_whitelist_free(w);
        return rc;
    }
    *out = w;
    return ROGTK_OK;
}

int barcode_correct(const void* handle, const DevCol& col, int ambiguous, const uint32_t* prior_counts, uint32_t* index,
                    uint8_t* status, uint32_t* exact_counts, uint32_t* counts, bool count_only, int64_t* totals5,
                    hipStream_t s) {
    const auto [offsets, ow, values, validity, voff, n] = col;
    const Whitelist* w = (const Whitelist*)handle;
    if (int rc = check_device(w)) return rc;
    const int64_t W = w->W;
    const bool reject = ambiguous == ROGTK_BC_REJECT;
    const bool own_exact = !exact_counts;
    Arena A;
    if (int rc = A.get(al(64) + (own_exact ? al((size_t)W * 4) : 0) +
                           (count_only ? 0 : al((size_t)n * 8) + al((size_t)n * 4) + al((size_t)n)),
                       s))
        return rc;
    unsigned long long* cnt = A.take<unsigned long long>(8);
    if (own_exact) exact_counts = A.take<uint32_t>(W);
    uint64_t* miss_code = count_only ? nullptr : A.take<uint64_t>(n);
    uint32_t* miss_row = count_only ? nullptr : A.take<uint32_t>(n);
    uint8_t* miss_unk = count_only ? nullptr : A.take<uint8_t>(n);
    ROGTK_HIP_CHECK(hipMemsetAsync(cnt, 0, 64, s));
    if (own_exact || !count_only) ROGTK_HIP_CHECK(hipMemsetAsync(exact_counts, 0, (size_t)W * 4, s));
    unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const View v = view_of(w);
    const dim3 b(kBlock);
    if (n > 0) {
        const dim3 g(grid_for(n, kTile, kExactBlocks));
        if (ow == 4)
            hipLaunchKernelGGL(k_bc_exact<4>, g, b, 0, s, offsets, values, validity, voff, n, v, index, status,
                               exact_counts, miss_code, miss_row, miss_unk, cnt);
        else
            hipLaunchKernelGGL(k_bc_exact<8>, g, b, 0, s, offsets, values, validity, voff, n, v, index, status,
                               exact_counts, miss_code, miss_row, miss_unk, cnt);
        ROGTK_HIP_CHECK(hipGetLastError());
    }
    if (!count_only) {
        if (counts) ROGTK_HIP_CHECK(hipMemcpyAsync(counts, exact_counts, (size_t)W * 4, hipMemcpyDeviceToDevice, s));
        ROGTK_HIP_CHECK(hipMemcpyAsync(h, cnt, 8, hipMemcpyDeviceToHost, s));
        ROGTK_HIP_CHECK(hipStreamSynchronize(s));
        const int64_t n_miss = (int64_t)h[0];
        if (n_miss > 0) {
            const uint32_t* prior = reject ? nullptr : prior_counts ? prior_counts : exact_counts;
            if (g_probe.load(std::memory_order_relaxed) & kBarcodeProbeLane)
                hipLaunchKernelGGL(k_bc_probe<true>, dim3(grid_for(n_miss, kBlock)), b, 0, s,
                                   (const uint64_t*)miss_code, (const uint32_t*)miss_row, (const uint8_t*)miss_unk,
                                   n_miss, v, prior, (int)reject, index, status, counts, cnt);
            else
                hipLaunchKernelGGL(k_bc_probe<false>, dim3(grid_for(n_miss, kWaves)), b, 0, s,
                                   (const uint64_t*)miss_code, (const uint32_t*)miss_row, (const uint8_t*)miss_unk,
                                   n_miss, v, prior, (int)reject, index, status, counts, cnt);
            ROGTK_HIP_CHECK(hipGetLastError());
        }
    }
    ROGTK_HIP_CHECK(hipMemcpyAsync(h, cnt, 64, hipMemcpyDeviceToHost, s));
    ROGTK_HIP_CHECK(hipStreamSynchronize(s));
    if (totals5)
        for (int k = 0; k < 5; ++k) totals5[k] = (int64_t)h[1 + k];
    return ROGTK_OK;
}

int barcode_corrected_temp(int64_t n, int64_t* bytes) {
    size_t scan_b = 0;
    ROGTK_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, (const int64_t*)nullptr, (int64_t*)nullptr,
                                                     n + 1, nullptr));
    *bytes = (int64_t)(al((size_t)(n + 1) * 8) + al(scan_b));
    return ROGTK_OK;
}

int barcode_corrected_measure(const void* handle, const uint8_t* status, int64_t n, int64_t* out_offsets, void* temp,
                              int64_t temp_bytes, hipStream_t s) {
    const Whitelist* w = (const Whitelist*)handle;
    int64_t need = 0;
    if (int rc = barcode_corrected_temp(n, &need)) return rc;
    ROGTK_REQUIRE(temp && temp_bytes >= need, ROGTK_E_INVALID, "barcode corrected: temp too small");
    int64_t* len = (int64_t*)temp;
    size_t scan_b = (size_t)need - al((size_t)(n + 1) * 8);
    hipLaunchKernelGGL(k_bc_lengths, dim3(grid_for(n + 1, kBlock)), dim3(kBlock), 0, s, status, n, w->L, len);
    ROGTK_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum((uint8_t*)temp + al((size_t)(n + 1) * 8), scan_b,
                                                     (const int64_t*)len, out_offsets, n + 1, s));
    return ROGTK_OK;
}

int barcode_corrected_fill(const void* handle, const uint32_t* index, const uint8_t* status, int64_t n,
                           const int64_t* out_offsets, uint8_t* out_values, hipStream_t s) {
    const Whitelist* w = (const Whitelist*)handle;
    if (n == 0) return ROGTK_OK;
    hipLaunchKernelGGL(k_bc_fill, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, index, status, n, w->L, w->by_row,
                       out_offsets, out_values);
    ROGTK_HIP_CHECK(hipGetLastError());
    return ROGTK_OK;
}

}  // namespace rogtk
