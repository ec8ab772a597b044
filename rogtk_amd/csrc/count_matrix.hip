// count_matrix.hip — the UMI count matrix on gfx950: for every (cell, feature)
// pair with at least one live row, the number of distinct molecule ids and the number of rows,
// entries ascending in (cell, feature), with the CSR row pointer over the cells.
//
//   cell[n], feature[n], molecule[n] u32; n_cells, n_features, n_molecules. A row is live when
//   each of its three ids is below its size; every other row (0xFFFFFFFF among them) is skipped.
//
// Every row has one u64 key, cell << (fb + mb) | feature << mb | molecule, with cb =
// bit_width(n_cells), fb = bit_width(n_features - 1), mb = bit_width(n_molecules - 1). A skipped
// row's key is n_cells << (fb + mb): it sorts after every live key and is known by its cell field.
//
//   pack    the keys, 16 bytes of every column per lane where the columns allow it
//   sort    hipcub radix sort of the keys over bits [0, cb + fb + mb)
//   flags   per sorted position: live, new molecule (key differs from its predecessor), new entry
//           (key >> mb differs); per tile the popcounts of the three ballots
//   scan    exclusive scan of the tile popcounts and the three totals (k_tile_scan of id_columns.h)
//   emit    every new-entry position i gets e = offset[tile] + rank in tile and writes the
//           entry's cell and feature, row_start[e] = i and mol_start[e] = new molecules before i
//   diff    n_reads[e] = row_start[e + 1] - row_start[e], n_umis[e] = mol_start[e + 1] -
//           mol_start[e]; the end of the last entry is the live-row / molecule total
//   indptr  one lower-bound binary search in entry_cell per cell
//
// No output atomics: an entry or a run of one molecule that crosses tile edges is a difference
// of two positions. The answer depends on the inputs alone. Enqueue-only: no allocation, no
// synchronisation, everything on the caller's stream.
#include <atomic>

#include <hipcub/hipcub.hpp>

#include "../../include/rogtk_count.h"
#include "id_columns.h"

namespace rogtk {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kSteps = 8;                     // 64-row steps per wave and tile
constexpr int kTile = kBlock * kSteps;        // 2048 sorted positions per flag / emit tile
constexpr int kWaveRows = 64 * kSteps;        // consecutive positions of one wave
constexpr int64_t kMaxSize = (1ll << 32) - 1;  // sizes are 0..2^32-1
constexpr size_t kTempAlign = 256;            // the call rounds temp up to this

std::atomic<int> g_phases{7};  // 1 pack | 2 sort | 4 flags .. indptr (measurements only)

typedef unsigned long long u64x2_t __attribute__((ext_vector_type(2)));

int bit_width(uint64_t v) {
    int b = 0;
    while (b < 64 && (v >> b)) ++b;
    return b;
}

// the key's fields; by value into every kernel
struct CountKey {
    int fm;       // fb + mb: the cell field starts here
    int mb;       // the feature field starts here
    int bits;     // cb + fb + mb
    uint32_t nc, nf, nm;
    unsigned long long fmask;  // (1 << fb) - 1
};

struct Widths {
    int cb, fb, mb;
};

Widths widths(int64_t nc, int64_t nf, int64_t nm) {
    return Widths{bit_width((uint64_t)nc), bit_width((uint64_t)(nf - 1)), bit_width((uint64_t)(nm - 1))};
}

CountKey make_key(int64_t nc, int64_t nf, int64_t nm) {
    const Widths w = widths(nc, nf, nm);
    CountKey k;
    k.fm = w.fb + w.mb;
    k.mb = w.mb;
    k.bits = w.cb + w.fb + w.mb;
    k.nc = (uint32_t)nc;
    k.nf = (uint32_t)nf;
    k.nm = (uint32_t)nm;
    k.fmask = (1ull << w.fb) - 1ull;  // fb <= 32
    return k;
}

__device__ __forceinline__ unsigned long long pack_key(uint32_t c, uint32_t f, uint32_t m, const CountKey& p) {
    if (c < p.nc && f < p.nf && m < p.nm)
        return ((unsigned long long)c << p.fm) | ((unsigned long long)f << p.mb) | (unsigned long long)m;
    return (unsigned long long)p.nc << p.fm;
}

// key[] is 16-byte aligned (the call aligns temp), so rows r0 .. r0 + 3 take two 16-byte stores
__global__ void __launch_bounds__(kBlock)
k_count_pack(const uint32_t* __restrict__ cell, const uint32_t* __restrict__ feature,
             const uint32_t* __restrict__ molecule, int64_t n, CountKey p, bool vec,
             unsigned long long* __restrict__ key) {
    const int64_t r0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 4;
    if (r0 >= n) return;
    uint32_t c[4], f[4], m[4];
    load4(cell, r0, n, vec, 0xFFFFFFFFu, c);
    load4(feature, r0, n, vec, 0xFFFFFFFFu, f);
    load4(molecule, r0, n, vec, 0xFFFFFFFFu, m);
    unsigned long long k[4];
    for (int j = 0; j < 4; ++j) k[j] = pack_key(c[j], f[j], m[j], p);
    if (r0 + 4 <= n) {
        u64x2_t a, b;
        a.x = k[0];
        a.y = k[1];
        b.x = k[2];
        b.y = k[3];
        *(u64x2_t*)(key + r0) = a;
        *(u64x2_t*)(key + r0 + 2) = b;
    } else {
        for (int j = 0; j < 4; ++j)
            if (r0 + j < n) key[r0 + j] = k[j];
    }
}

// The three flags of sorted position i, one lane per position of a 64-row step. Every lane of the
// wave calls this (the shuffle); the predecessor of lane 0 is a plain global load.
__device__ __forceinline__ void flags_at(const unsigned long long* __restrict__ key, int64_t i, int64_t n, int lane,
                                         const CountKey& p, unsigned long long& k, bool& live, bool& new_mol,
                                         bool& new_entry) {
    const bool in = i < n;
    k = in ? key[i] : 0ull;
    unsigned long long prev = __shfl_up(k, 1);
    if (lane == 0) prev = (in && i > 0) ? key[i - 1] : 0ull;
    live = in && (k >> p.fm) < (unsigned long long)p.nc;
    new_mol = live && (i == 0 || k != prev);
    new_entry = live && (i == 0 || (k >> p.mb) != (prev >> p.mb));
}

// per tile the popcounts of new_entry, new_mol and live: counts[0 .. nt), [nt .. 2 nt), [2 nt .. 3 nt)
__global__ void __launch_bounds__(kBlock)
k_count_flags(const unsigned long long* __restrict__ key, int64_t n, CountKey p, int64_t nt,
              uint32_t* __restrict__ counts) {
    __shared__ uint32_t wsum[3][kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w0 = (int64_t)blockIdx.x * kTile + (int64_t)wave * kWaveRows;
    uint32_t ce = 0, cm = 0, cl = 0;
    for (int s = 0; s < kSteps; ++s) {
        const int64_t i = w0 + (int64_t)s * 64 + lane;
        if (i - lane >= n) break;  // the whole wave
        unsigned long long k;
        bool live, nm, ne;
        flags_at(key, i, n, lane, p, k, live, nm, ne);
        ce += (uint32_t)__popcll(__ballot(ne));
        cm += (uint32_t)__popcll(__ballot(nm));
        cl += (uint32_t)__popcll(__ballot(live));
    }
    if (lane == 0) {
        wsum[0][wave] = ce;
        wsum[1][wave] = cm;
        wsum[2][wave] = cl;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        uint32_t t = 0;
        for (int w = 0; w < kWaves; ++w) t += wsum[threadIdx.x][w];
        counts[(int64_t)threadIdx.x * nt + blockIdx.x] = t;
    }
}

// Every new-entry position of the tile: its entry index from the tile's offset and its rank in the
// tile. entry_cell / entry_feature below capacity; the two temporaries up to capacity itself (the
// end of a last entry that was cut off).
__global__ void __launch_bounds__(kBlock)
k_count_emit(const unsigned long long* __restrict__ key, int64_t n, CountKey p, int64_t nt,
             const uint32_t* __restrict__ offs, int64_t capacity, uint32_t* __restrict__ entry_cell,
             uint32_t* __restrict__ entry_feature, uint32_t* __restrict__ row_start, uint32_t* __restrict__ mol_start) {
    __shared__ uint32_t wsum[2][kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w0 = (int64_t)blockIdx.x * kTile + (int64_t)wave * kWaveRows;
    unsigned long long k[kSteps], me[kSteps], mm[kSteps];
    uint32_t ce = 0, cm = 0;
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        const int64_t i = w0 + (int64_t)s * 64 + lane;
        bool live, nm, ne;
        flags_at(key, i, n, lane, p, k[s], live, nm, ne);
        me[s] = __ballot(ne);
        mm[s] = __ballot(nm);
        ce += (uint32_t)__popcll(me[s]);
        cm += (uint32_t)__popcll(mm[s]);
    }
    if (lane == 0) {
        wsum[0][wave] = ce;
        wsum[1][wave] = cm;
    }
    __syncthreads();
    int64_t e0 = (int64_t)offs[blockIdx.x];
    uint32_t m0 = offs[nt + blockIdx.x];
    for (int w = 0; w < wave; ++w) {
        e0 += wsum[0][w];
        m0 += wsum[1][w];
    }
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
        if ((me[s] >> lane) & 1ull) {
            const int64_t e = e0 + __popcll(me[s] & below);
            if (e <= capacity) {
                row_start[e] = (uint32_t)(w0 + (int64_t)s * 64 + lane);
                mol_start[e] = m0 + (uint32_t)__popcll(mm[s] & below);
                if (e < capacity) {
                    entry_cell[e] = (uint32_t)(k[s] >> p.fm);
                    entry_feature[e] = (uint32_t)((k[s] >> p.mb) & p.fmask);
                }
            }
        }
        e0 += __popcll(me[s]);
        m0 += (uint32_t)__popcll(mm[s]);
    }
}

// the written entries, min(totals[0], capacity) of them (grid-stride)
__global__ void __launch_bounds__(kBlock)
k_count_diff(const int64_t* __restrict__ totals, int64_t capacity, const uint32_t* __restrict__ row_start,
             const uint32_t* __restrict__ mol_start, uint32_t* __restrict__ n_umis, uint32_t* __restrict__ n_reads) {
    const int64_t entries = totals[0];
    const int64_t m = entries < capacity ? entries : capacity;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < m; e += (int64_t)gridDim.x * kBlock) {
        const bool last = e + 1 == entries;  // its end is no entry's start: the totals
        const uint32_t r1 = last ? (uint32_t)totals[1] : row_start[e + 1];
        const uint32_t m1 = last ? (uint32_t)totals[2] : mol_start[e + 1];
        n_umis[e] = m1 - mol_start[e];
        if (n_reads) n_reads[e] = r1 - row_start[e];
    }
}

// indptr[c] = the first written entry whose cell is >= c, c in 0..n_cells
__global__ void __launch_bounds__(kBlock)
k_count_indptr(const int64_t* __restrict__ totals, int64_t capacity, const uint32_t* __restrict__ entry_cell,
               int64_t n_cells, int64_t* __restrict__ indptr) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c > n_cells) return;
    const int64_t entries = totals[0];
    int64_t lo = 0, hi = entries < capacity ? entries : capacity;
    for (int step = 0; step < 32 && lo < hi; ++step) {  // hi < 2^31
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)entry_cell[mid] < c)
            lo = mid + 1;
        else
            hi = mid;
    }
    indptr[c] = lo;
}

// planes {new entry, new molecule, live}: offsets for the first two, totals = {entries, live, molecules}
constexpr auto k_count_scan = k_tile_scan<2, 0, 2, 1>;

struct CountLayout {
    size_t off_key, off_sorted, off_cub, off_counts, off_offs, off_row, off_mol, total;
    size_t cub_bytes;
    int64_t tiles;
};

// The hipcub query launches nothing and is taken for the widest key, so the size depends on n and
// capacity alone. It asks the runtime for the device's architecture: in a machine without a device
// it fails, and the size is then an estimate (a third key array and 4 bytes per row of digit
// counts), good for sizing a request but not for a call, which such a machine cannot make.
int count_layout(int64_t n, int64_t capacity, CountLayout* out) {
    CountLayout p;
    p.tiles = (n + kTile - 1) / kTile;
    p.cub_bytes = 0;
    if (n > 0 &&
        hipcub::DeviceRadixSort::SortKeys(nullptr, p.cub_bytes, (const unsigned long long*)nullptr,
                                          (unsigned long long*)nullptr, (int)n, 0, 64) != hipSuccess) {
        (void)hipGetLastError();
        p.cub_bytes = (size_t)n * 12 + (1u << 20);
    }
    const int64_t slots = std::min(capacity, n) + 1;  // entries <= n
    Carve c;
    p.off_key = c.take((size_t)n * 8);
    p.off_sorted = c.take((size_t)n * 8);
    p.off_cub = c.take(p.cub_bytes);
    p.off_counts = c.take((size_t)p.tiles * 3 * 4);
    p.off_offs = c.take((size_t)p.tiles * 2 * 4);
    p.off_row = c.take((size_t)slots * 4);
    p.off_mol = c.take((size_t)slots * 4);
    p.total = c.total + kTempAlign;  // room to round the caller's pointer up
    *out = p;
    return ROGTK_OK;
}

struct CountArgs {
    const uint32_t *cell, *feature, *molecule;
    int64_t n, n_cells, n_features, n_molecules;
    uint32_t *entry_cell, *entry_feature, *n_umis, *n_reads;
    int64_t capacity;
    int64_t* indptr;
    int64_t* totals;
};

bool no_entries(const CountArgs& a) { return a.n == 0 || a.n_cells == 0 || a.n_features == 0 || a.n_molecules == 0; }

// The argument rules of both levels (include/rogtk_count.h), before any device work. The width
// of the key is decided here, from the three sizes alone.
int check_sizes(const char* name, int64_t n, int64_t nc, int64_t nf, int64_t nm) {
    if (int rc = check_rows(name, n)) return rc;
    ROGTK_REQUIRE(nc >= 0 && nc <= kMaxSize, ROGTK_E_INVALID, "%s: n_cells %lld outside 0..2^32-1", name,
                  (long long)nc);
    ROGTK_REQUIRE(nf >= 0 && nf <= kMaxSize, ROGTK_E_INVALID, "%s: n_features %lld outside 0..2^32-1", name,
                  (long long)nf);
    ROGTK_REQUIRE(nm >= 0 && nm <= kMaxSize, ROGTK_E_INVALID, "%s: n_molecules %lld outside 0..2^32-1", name,
                  (long long)nm);
    if (nc > 0 && nf > 0 && nm > 0) {
        const Widths w = widths(nc, nf, nm);
        ROGTK_REQUIRE(w.cb + w.fb + w.mb <= 64, ROGTK_E_UNSUPPORTED,
                      "%s: the key needs %d bits (cells %d + features %d + molecules %d), at most 64", name,
                      w.cb + w.fb + w.mb, w.cb, w.fb, w.mb);
    }
    return ROGTK_OK;
}

int check_count(const char* name, const CountArgs& a) {
    if (int rc = check_sizes(name, a.n, a.n_cells, a.n_features, a.n_molecules)) return rc;
    ROGTK_REQUIRE(a.capacity >= 0, ROGTK_E_INVALID, "%s: capacity %lld is negative", name, (long long)a.capacity);
    ROGTK_REQUIRE(a.totals, ROGTK_E_INVALID, "%s: totals is NULL", name);
    ROGTK_REQUIRE(a.n == 0 || a.cell, ROGTK_E_INVALID, "%s: cell is NULL", name);
    ROGTK_REQUIRE(a.n == 0 || a.feature, ROGTK_E_INVALID, "%s: feature is NULL", name);
    ROGTK_REQUIRE(a.n == 0 || a.molecule, ROGTK_E_INVALID, "%s: molecule is NULL", name);
    ROGTK_REQUIRE(a.capacity == 0 || a.entry_cell, ROGTK_E_INVALID, "%s: entry_cell is NULL", name);
    ROGTK_REQUIRE(a.capacity == 0 || a.entry_feature, ROGTK_E_INVALID, "%s: entry_feature is NULL", name);
    ROGTK_REQUIRE(a.capacity == 0 || a.n_umis, ROGTK_E_INVALID, "%s: n_umis is NULL", name);
    return ROGTK_OK;
}

// The arguments are checked by the caller; temp is large enough for count_layout(n, capacity).
int launch_count_matrix(const CountArgs& a, const CountLayout& p, void* temp, hipStream_t s) {
    if (no_entries(a)) {
        ROGTK_HIP_CHECK(hipMemsetAsync(a.totals, 0, 3 * sizeof(int64_t), s));
        if (a.indptr) ROGTK_HIP_CHECK(hipMemsetAsync(a.indptr, 0, (size_t)(a.n_cells + 1) * 8, s));
        return ROGTK_OK;
    }
    // the pieces start at multiples of 256 from a 256-byte aligned base inside temp
    uint8_t* t = (uint8_t*)(((uintptr_t)temp + kTempAlign - 1) / kTempAlign * kTempAlign);
    unsigned long long* key = (unsigned long long*)(t + p.off_key);
    unsigned long long* sorted = (unsigned long long*)(t + p.off_sorted);
    uint32_t* counts = (uint32_t*)(t + p.off_counts);
    uint32_t* offs = (uint32_t*)(t + p.off_offs);
    uint32_t* row_start = (uint32_t*)(t + p.off_row);
    uint32_t* mol_start = (uint32_t*)(t + p.off_mol);
    const CountKey k = make_key(a.n_cells, a.n_features, a.n_molecules);
    const int64_t n = a.n;
    const int phases = g_phases.load();
    const dim3 b(kBlock);
    if (phases & 1) {
        const bool vec = (((uintptr_t)a.cell | (uintptr_t)a.feature | (uintptr_t)a.molecule) & 15u) == 0;
        hipLaunchKernelGGL(k_count_pack, dim3(grid_for(n, kBlock * 4)), b, 0, s, a.cell, a.feature, a.molecule, n, k,
                           vec, key);
    }
    if (phases & 2) {
        size_t tb = p.cub_bytes;
        ROGTK_HIP_CHECK(hipcub::DeviceRadixSort::SortKeys(t + p.off_cub, tb, (const unsigned long long*)key, sorted,
                                                          (int)n, 0, k.bits, s));
    }
    if (phases & 4) {
        const dim3 g((unsigned)p.tiles);
        hipLaunchKernelGGL(k_count_flags, g, b, 0, s, sorted, n, k, p.tiles, counts);
        hipLaunchKernelGGL(k_count_scan, dim3(1), dim3(kScanBlock), 0, s, counts, p.tiles, offs, a.totals);
        hipLaunchKernelGGL(k_count_emit, g, b, 0, s, sorted, n, k, p.tiles, offs, a.capacity, a.entry_cell,
                           a.entry_feature, row_start, mol_start);
        const int64_t most = std::min(a.capacity, n);  // entries <= n
        if (most > 0)
            hipLaunchKernelGGL(k_count_diff, dim3(grid_for(most, kBlock, 1 << 16)), b, 0, s, a.totals, a.capacity,
                               row_start, mol_start, a.n_umis, a.n_reads);
        if (a.indptr)
            hipLaunchKernelGGL(k_count_indptr, dim3(grid_for(a.n_cells + 1, kBlock)), b, 0, s, a.totals, a.capacity,
                               a.entry_cell, a.n_cells, a.indptr);
    }
    ROGTK_HIP_CHECK(hipGetLastError());
    return ROGTK_OK;
}

}  // namespace
}  // namespace rogtk

// ------------------------------------------------------------------ C ABI
// The entries live in a library of their own, rogtk_amd/_count/librogtk_count.so.
using namespace rogtk;

extern "C" {

int rogtk_count_matrix_temp_bytes(int64_t n, int64_t n_cells, int64_t n_features, int64_t n_molecules,
                                  int64_t capacity, int64_t* bytes) {
    ROGTK_REQUIRE(bytes, ROGTK_E_INVALID, "count_matrix_temp_bytes: NULL bytes");
    if (int rc = check_sizes("count_matrix_temp_bytes", n, n_cells, n_features, n_molecules)) return rc;
    ROGTK_REQUIRE(capacity >= 0, ROGTK_E_INVALID, "count_matrix_temp_bytes: capacity %lld is negative",
                  (long long)capacity);
    CountLayout p;
    if (int rc = count_layout(n, capacity, &p)) return rc;
    *bytes = (int64_t)p.total;
    return ROGTK_OK;
}

int rogtk_count_matrix_geometry(int64_t* out2) {
    ROGTK_REQUIRE(out2, ROGTK_E_INVALID, "count_matrix_geometry: NULL argument");
    out2[0] = kTile;
    out2[1] = kScanBlock;
    return ROGTK_OK;
}

int rogtk_count_matrix_set_phases(int phases) {
    ROGTK_REQUIRE(phases >= 1 && phases <= 7, ROGTK_E_INVALID, "count_matrix phases %d must be a mask in 1..7",
                  phases);
    g_phases.store(phases);
    return ROGTK_OK;
}

int rogtk_count_matrix(const uint32_t* cell, const uint32_t* feature, const uint32_t* molecule, int64_t n,
                       int64_t n_cells, int64_t n_features, int64_t n_molecules, uint32_t* entry_cell,
                       uint32_t* entry_feature, uint32_t* n_umis, uint32_t* n_reads, int64_t capacity, int64_t* indptr,
                       int64_t* totals, void* temp, int64_t temp_bytes, void* stream) {
    const CountArgs a{cell,       feature, molecule, n,        n_cells, n_features, n_molecules, entry_cell,
                      entry_feature, n_umis,  n_reads,  capacity, indptr,  totals};
    if (int rc = check_count("count_matrix", a)) return rc;
    ROGTK_REQUIRE(temp, ROGTK_E_INVALID, "count_matrix: temp is NULL");
    ROGTK_REQUIRE(((uintptr_t)temp & 7u) == 0, ROGTK_E_INVALID, "count_matrix: temp is not 8-byte aligned");
    CountLayout p;
    if (int rc = count_layout(n, capacity, &p)) return rc;
    ROGTK_REQUIRE(temp_bytes >= (int64_t)p.total, ROGTK_E_INVALID,
                  "count_matrix: temp_bytes %lld too small (need %lld)", (long long)temp_bytes, (long long)p.total);
    return launch_count_matrix(a, p, temp, (hipStream_t)stream);
}

int rogtk_count_matrix_host(const uint32_t* cell, const uint32_t* feature, const uint32_t* molecule, int64_t n,
                            int64_t n_cells, int64_t n_features, int64_t n_molecules, uint32_t* entry_cell,
                            uint32_t* entry_feature, uint32_t* n_umis, uint32_t* n_reads, int64_t capacity,
                            int64_t* indptr, int64_t* totals) {
    if (int rc = check_sizes("count_matrix_host", n, n_cells, n_features, n_molecules)) return rc;
    if (capacity < 0) {  // min(n, n_cells * n_features), the product not formed where it would pass n
        if (n_cells == 0 || n_features == 0)
            capacity = 0;
        else
            capacity = n_cells > n / n_features ? n : n_cells * n_features;
    }
    const CountArgs h{cell,       feature, molecule, n,        n_cells, n_features, n_molecules, entry_cell,
                      entry_feature, n_umis,  n_reads,  capacity, indptr,  totals};
    if (int rc = check_count("count_matrix_host", h)) return rc;
    CountLayout p;
    if (int rc = count_layout(n, capacity, &p)) return rc;
    // one allocation, the whole call on the default stream: the columns, the outputs, temp
    const int64_t cap = std::min(capacity, n);  // entries <= n: what the device can write
    HostCall m;
    const size_t o_cell = m.take((size_t)n * 4), o_feat = m.take((size_t)n * 4), o_mol = m.take((size_t)n * 4),
                 o_ec = m.take((size_t)cap * 4), o_ef = m.take((size_t)cap * 4), o_nu = m.take((size_t)cap * 4),
                 o_nr = m.take((size_t)cap * 4), o_ip = m.take(indptr ? (size_t)(n_cells + 1) * 8 : 0),
                 o_tot = m.take(24), o_temp = m.take(p.total);
    if (int rc = m.open("librogtk_count")) return rc;
    if (int rc = m.in(o_cell, cell, (size_t)n * 4)) return rc;
    if (int rc = m.in(o_feat, feature, (size_t)n * 4)) return rc;
    if (int rc = m.in(o_mol, molecule, (size_t)n * 4)) return rc;
    CountArgs a = h;
    a.cell = m.at<uint32_t>(o_cell);
    a.feature = m.at<uint32_t>(o_feat);
    a.molecule = m.at<uint32_t>(o_mol);
    a.entry_cell = m.at<uint32_t>(o_ec);
    a.entry_feature = m.at<uint32_t>(o_ef);
    a.n_umis = m.at<uint32_t>(o_nu);
    a.n_reads = n_reads ? m.at<uint32_t>(o_nr) : nullptr;
    a.capacity = cap;  // an entry index never reaches n, so the device sees the same cut
    a.indptr = indptr ? m.at<int64_t>(o_ip) : nullptr;
    a.totals = m.at<int64_t>(o_tot);
    if (int rc = launch_count_matrix(a, p, m.at<void>(o_temp), nullptr)) return rc;
    if (int rc = m.out(totals, o_tot, 24)) return rc;
    ROGTK_REQUIRE(totals[0] >= 0 && totals[0] <= n, ROGTK_E_HIP, "count_matrix_host: %lld entries outside 0..%lld",
                  (long long)totals[0], (long long)n);
    const size_t wrote = (size_t)std::min(totals[0], cap) * 4;
    if (int rc = m.out(entry_cell, o_ec, wrote)) return rc;
    if (int rc = m.out(entry_feature, o_ef, wrote)) return rc;
    if (int rc = m.out(n_umis, o_nu, wrote)) return rc;
    if (int rc = m.out(n_reads, o_nr, wrote)) return rc;
    return m.out(indptr, o_ip, (size_t)(n_cells + 1) * 8);
}

}  // extern "C"
