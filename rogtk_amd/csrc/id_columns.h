// id_columns.h — what the two libraries that work on plain u32 id columns share (dedup.hip,
// count_matrix.hip): the 16-byte column load, the wave scan, the scan of per-tile
// popcounts, the row-count rule and the frame of a Level-2 host call. Header-only, not installed.
// Everything has internal linkage: both libraries live in one process, each with its own kernels.
#pragma once

#include "column_util.h"

namespace rogtk {
namespace {

constexpr int kScanBlock = 1024;  // the tile scan's one workgroup

// rows r0 .. r0 + 3 of p (one 16-byte load when the column allows it), `fill` past n
__device__ __forceinline__ void load4(const uint32_t* __restrict__ p, int64_t r0, int64_t n, bool vec, uint32_t fill,
                                      uint32_t (&v)[4]) {
    if (vec && r0 + 4 <= n) {
        const u32x4_t q = stream_load((const u32x4_t*)(p + r0));
        v[0] = q.x;
        v[1] = q.y;
        v[2] = q.z;
        v[3] = q.w;
    } else {
        for (int k = 0; k < 4; ++k) v[k] = r0 + k < n ? p[r0 + k] : fill;
    }
}

// inclusive scan of s over the 64 lanes of a wave; every lane calls it
__device__ __forceinline__ uint32_t wave_scan(uint32_t s, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(s, d);
        if (lane >= d) s += u;
    }
    return s;
}

// The scan of per-tile popcounts, launched as <<<1, kScanBlock>>>. counts holds one plane of nt
// u32 per entry of TOTAL, plane a at counts + a * nt. Planes 0 .. OFFS - 1 get their exclusive
// offsets, laid out the same way in offs; totals[j] is the sum of plane TOTAL[j]. One workgroup
// walks the tiles in chunks of kScanBlock and carries the sums in registers: no look-back,
// nothing spins, and a chunk's offsets depend on nothing but the counts before it.
template <int OFFS, int... TOTAL>
__global__ void __launch_bounds__(kScanBlock)
k_tile_scan(const uint32_t* __restrict__ counts, int64_t nt, uint32_t* __restrict__ offs,
            int64_t* __restrict__ totals) {
    constexpr int kPlanes = sizeof...(TOTAL);
    static_assert(OFFS <= kPlanes, "offsets for planes that exist");
    __shared__ uint32_t wtot[kPlanes][kScanBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry[kPlanes] = {};
    for (int64_t base = 0; base < nt; base += kScanBlock) {
        const int64_t i = base + threadIdx.x;
        uint32_t v[kPlanes], s[kPlanes];
        for (int a = 0; a < kPlanes; ++a) {
            v[a] = i < nt ? counts[(int64_t)a * nt + i] : 0u;
            s[a] = wave_scan(v[a], lane);
        }
        if (lane == 63)
            for (int a = 0; a < kPlanes; ++a) wtot[a][wave] = s[a];
        __syncthreads();
        for (int a = 0; a < kPlanes; ++a) {
            uint32_t before = 0, total = 0;
            for (int k = 0; k < kScanBlock / 64; ++k) {
                const uint32_t t = wtot[a][k];
                if (k < wave) before += t;
                total += t;
            }
            if (a < OFFS && i < nt) offs[(int64_t)a * nt + i] = carry[a] + before + s[a] - v[a];
            carry[a] += total;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int j = 0;
        ((totals[j++] = (int64_t)carry[TOTAL]), ...);
    }
}

// the row-count rule of every entry: 0 <= n < 2^31
inline int check_rows(const char* name, int64_t n) {
    ROGTK_REQUIRE(n >= 0 && n < (1ll << 31), ROGTK_E_INVALID, "%s: n %lld outside 0..2^31-1", name, (long long)n);
    return ROGTK_OK;
}

// One Level-2 host call: every device piece the call needs (the columns, the outputs, temp) is
// taken from one hipMalloc, released on every way out. The call runs on the default stream, so
// the blocking copies are ordered around the kernels: in() before the launch, out() behind it.
struct HostCall {
    Carve need;
    uint8_t* d = nullptr;
    ~HostCall() {
        if (d) (void)hipFree(d);
    }
    size_t take(size_t bytes) { return need.take(bytes); }
    // after the last take(): refuses a machine without a device, then allocates
    int open(const char* library) {
        int devices = 0;
        if (hipGetDeviceCount(&devices) != hipSuccess || devices <= 0) {
            set_error("no HIP device available (%s needs an MI355X / gfx950 GPU)", library);
            return ROGTK_E_NODEVICE;
        }
        ROGTK_HIP_CHECK(hipMalloc((void**)&d, need.total));
        return ROGTK_OK;
    }
    template <class T>
    T* at(size_t off) const {
        return (T*)(d + off);
    }
    // the blocking copies; none for a NULL host pointer (an argument left out) or for 0 bytes
    int in(size_t off, const void* host, size_t bytes) {
        if (host && bytes) ROGTK_HIP_CHECK(hipMemcpy(d + off, host, bytes, hipMemcpyHostToDevice));
        return ROGTK_OK;
    }
    int out(void* host, size_t off, size_t bytes) {
        if (host && bytes) ROGTK_HIP_CHECK(hipMemcpy(host, d + off, bytes, hipMemcpyDeviceToHost));
        return ROGTK_OK;
    }
};

}  // namespace
}  // namespace rogtk
