// level2.hip — the definitions of what level2.h declares: the per-thread
// device context of the level-2 (host Arrow buffer) entry points and its transfers, the upload
// of a host column, the longest-row helpers, the checks those entries share and the writer of
// a rogtk_str_result. The entries themselves are in capi.hip, umi_api.hip, strings.hip and
// fuzzy.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "level2.h"

namespace rogtk {
namespace {

constexpr size_t kStageChunk = (size_t)32 << 20;
constexpr size_t kSmallCopy = (size_t)64 << 10;  // below this a host memcpy costs less than asking what the memory is

int host_copy_threads() {
    static const int t = [] {
        const char* e = getenv("OMP_NUM_THREADS");
        int v = e ? atoi(e) : 0;
        const int hw = (int)std::thread::hardware_concurrency();
        if (v <= 0) v = hw > 0 ? hw : 4;
        return std::max(1, std::min(v, 8));
    }();
    return t;
}

void par_memcpy(void* dst, const void* src, size_t bytes) {
    const int t = bytes >= ((size_t)4 << 20) ? host_copy_threads() : 1;
    if (t <= 1) {
        std::memcpy(dst, src, bytes);
        return;
    }
    std::vector<std::thread> pool;
    const size_t per = (bytes / t + 4095) / 4096 * 4096;
    for (int k = 0; k < t; ++k) {
        const size_t a = std::min(bytes, per * k), b = std::min(bytes, per * (k + 1));
        if (a < b) pool.emplace_back([=] { std::memcpy((uint8_t*)dst + a, (const uint8_t*)src + a, b - a); });
    }
    for (auto& th : pool) th.join();
}

bool is_pinned(const void* p) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

thread_local std::unique_ptr<HostCtx> t_ctx;

// Longest row of a device column (irregular rows' radix-sort / byte-path width).
template <class O>
__global__ void k_max_len(const O* __restrict__ off, int64_t n, unsigned long long* out) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long m = 0;
    if (r < n) m = (unsigned long long)((int64_t)off[r + 1] - (int64_t)off[r]);
    for (int d = 32; d; d >>= 1) m = max(m, (unsigned long long)__shfl_xor(m, d));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

}  // namespace

int require_device() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        set_error("no HIP device available (librogtk_hip needs an MI355X / gfx950 GPU)");
        return ROGTK_E_NODEVICE;
    }
    return ROGTK_OK;
}

HostCtx::~HostCtx() {
    for (int k = 0; k < 2; ++k) {
        if (pin[k]) hipHostFree(pin[k]);
        if (ev[k]) hipEventDestroy(ev[k]);
    }
    if (stream) hipStreamDestroy(stream);
}

int HostCtx::staging() {
    for (int k = 0; k < 2; ++k) {
        if (!pin[k]) ROGTK_HIP_CHECK(hipHostMalloc(&pin[k], kStageChunk, hipHostMallocDefault));
        if (!ev[k]) ROGTK_HIP_CHECK(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
    }
    return ROGTK_OK;
}

int HostCtx::d2h(void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return ROGTK_OK;
    // every path below waits for the stream, and with it for the small uploads out of pin[0]
    // (a copy into pin[0] here is ordered behind them by the stream)
    if (bytes > kSmallCopy && is_pinned(dst)) {
        ROGTK_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
        ROGTK_HIP_CHECK(hipStreamSynchronize(stream));
        pin_used = 0;
        return ROGTK_OK;
    }
    if (int rc = staging()) return rc;
    size_t prev_off = 0, prev_len = 0;
    int k = 0;
    for (size_t off = 0; off < bytes; off += kStageChunk, k ^= 1) {
        const size_t len = std::min(kStageChunk, bytes - off);
        ROGTK_HIP_CHECK(hipMemcpyAsync(pin[k], (const uint8_t*)src + off, len, hipMemcpyDeviceToHost, stream));
        ROGTK_HIP_CHECK(hipEventRecord(ev[k], stream));
        if (off > 0) {  // the previous chunk: out of its staging buffer while this one moves
            ROGTK_HIP_CHECK(hipEventSynchronize(ev[k ^ 1]));
            par_memcpy((uint8_t*)dst + prev_off, pin[k ^ 1], prev_len);
        }
        prev_off = off;
        prev_len = len;
    }
    ROGTK_HIP_CHECK(hipEventSynchronize(ev[k ^ 1]));
    pin_used = 0;
    par_memcpy((uint8_t*)dst + prev_off, pin[k ^ 1], prev_len);
    return ROGTK_OK;
}

int HostCtx::h2d(void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return ROGTK_OK;
    if (bytes <= kSmallCopy) {
        if (int rc = staging()) return rc;
        if (pin_used + bytes > kStageChunk) {
            ROGTK_HIP_CHECK(hipStreamSynchronize(stream));
            pin_used = 0;
        }
        uint8_t* at = (uint8_t*)pin[0] + pin_used;
        std::memcpy(at, src, bytes);
        ROGTK_HIP_CHECK(hipMemcpyAsync(dst, at, bytes, hipMemcpyHostToDevice, stream));
        pin_used += (bytes + 255) / 256 * 256;
        return ROGTK_OK;
    }
    if (is_pinned(src)) {
        ROGTK_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
        return ROGTK_OK;
    }
    if (int rc = staging()) return rc;
    if (pin_used) {  // small uploads may still read pin[0]
        ROGTK_HIP_CHECK(hipStreamSynchronize(stream));
        pin_used = 0;
    }
    int k = 0;
    int64_t i = 0;
    for (size_t off = 0; off < bytes; off += kStageChunk, k ^= 1, ++i) {
        const size_t len = std::min(kStageChunk, bytes - off);
        if (i >= 2) ROGTK_HIP_CHECK(hipEventSynchronize(ev[k]));  // its DMA of two chunks ago is done
        par_memcpy(pin[k], (const uint8_t*)src + off, len);
        ROGTK_HIP_CHECK(hipMemcpyAsync((uint8_t*)dst + off, pin[k], len, hipMemcpyHostToDevice, stream));
        ROGTK_HIP_CHECK(hipEventRecord(ev[k], stream));
    }
    // the staging buffers are reused by the next transfer only after these DMAs: every
    // later use first waits on the events above (or the stream is synchronised)
    ROGTK_HIP_CHECK(hipStreamSynchronize(stream));
    return ROGTK_OK;
}

int host_ctx(HostCtx** out) {
    if (int rc = require_device()) return rc;
    int dev = 0;
    ROGTK_HIP_CHECK(hipGetDevice(&dev));
    if (!t_ctx || t_ctx->device != dev) {
        t_ctx.reset(new HostCtx());
        t_ctx->device = dev;
        ROGTK_HIP_CHECK(hipStreamCreateWithFlags(&t_ctx->stream, hipStreamNonBlocking));
    }
    *out = t_ctx.get();
    return ROGTK_OK;
}

int launch_max_len(const void* offsets, int ow, int64_t n, unsigned long long* slot, hipStream_t s) {
    const dim3 g((unsigned)((n + 255) / 256));
    if (ow == 4)
        hipLaunchKernelGGL(k_max_len<int32_t>, g, dim3(256), 0, s, (const int32_t*)offsets, n, slot);
    else
        hipLaunchKernelGGL(k_max_len<int64_t>, g, dim3(256), 0, s, (const int64_t*)offsets, n, slot);
    ROGTK_HIP_CHECK(hipGetLastError());
    return ROGTK_OK;
}

int column_max_len(const void* offsets, int ow, int64_t n, unsigned long long* slot, hipStream_t s, int64_t* out) {
    ROGTK_HIP_CHECK(hipMemsetAsync(slot, 0, 8, s));
    if (int rc = launch_max_len(offsets, ow, n, slot, s)) return rc;
    unsigned long long h = 0;
    ROGTK_HIP_CHECK(hipMemcpyAsync(&h, slot, 8, hipMemcpyDeviceToHost, s));
    ROGTK_HIP_CHECK(hipStreamSynchronize(s));
    *out = (int64_t)h;
    return ROGTK_OK;
}

int device_max_len(HostCtx* c, const DevCol& col, int64_t* out) {
    if (int rc = c->nirr.ensure(16)) return rc;
    return column_max_len(col.offsets, col.ow, col.n, c->nirr.as<unsigned long long>() + 1, c->stream, out);
}

int check_rows_and_clusters(const char* name, int64_t n, int64_t n_clusters) {
    ROGTK_REQUIRE(n >= 0 && n < (1ll << 31), ROGTK_E_UNSUPPORTED, "%s: n %lld outside 0..2^31-1", name, (long long)n);
    ROGTK_REQUIRE(n_clusters >= 0 && n_clusters < (1ll << 32) - 1, ROGTK_E_INVALID, "%s: bad n_clusters %lld", name,
                  (long long)n_clusters);
    return ROGTK_OK;
}

int upload_col(HostCtx* c, int slot, const HostCol& h, DevCol* out) {
    ColBufs& b = c->in[slot];
    const int64_t n = h.n, base = h.off0(), end = h.off(n);
    ROGTK_REQUIRE(end <= h.values_len || h.values_len < 0, ROGTK_E_INVALID,
                  "offsets reference %lld bytes but values_len is %lld", (long long)end, (long long)h.values_len);
    ROGTK_REQUIRE(base >= 0 && end >= base, ROGTK_E_INVALID, "offsets reference bytes outside values");
    const void* offs = h.offsets;
    int ow = h.ow;
    std::vector<int64_t> rebased;  // h2d has copied it (or waited for its copy) on return
    if (base != 0) {
        rebased.resize((size_t)n + 1);
        for (int64_t r = 0; r <= n; ++r) rebased[r] = h.off(r) - base;
        offs = rebased.data();
        ow = 8;
    }
    if (int rc = b.offsets.ensure((size_t)(n + 1) * ow)) return rc;
    if (int rc = c->h2d(b.offsets.p, offs, (size_t)(n + 1) * ow)) return rc;
    if (int rc = b.values.ensure((size_t)std::max<int64_t>(end - base, 1))) return rc;
    if (int rc = c->h2d(b.values.p, h.values + base, (size_t)(end - base))) return rc;
    if (h.validity) {
        const size_t vb = (size_t)((h.voff + n + 7) / 8);
        if (int rc = b.validity.ensure(vb)) return rc;
        if (int rc = c->h2d(b.validity.p, h.validity, vb)) return rc;
    }
    *out = DevCol(b.offsets.p, ow, b.values.as<uint8_t>(), h.validity ? b.validity.as<uint8_t>() : nullptr, h.voff, n);
    return ROGTK_OK;
}

int stage_uploaded(HostCtx* c, const DevCol& col, int L, int64_t* n_irr, hipStream_t s) {
    const int64_t n = col.n, words = (n + 63) / 64;
    if (c->codes.ensure((size_t)std::max<int64_t>(n, 4) * 4) != ROGTK_OK ||
        c->regbits.ensure((size_t)std::max<int64_t>(words, 1) * 8) != ROGTK_OK ||
        c->irr.ensure((size_t)std::max<int64_t>(n, 1) * 8) != ROGTK_OK || c->nirr.ensure(16) != ROGTK_OK)
        return ROGTK_E_HIP;
    ROGTK_HIP_CHECK(hipMemsetAsync(c->nirr.p, 0, 16, s));
    if (int rc = launch_stage(col.offsets, col.ow, col.values, col.validity, col.voff, n, L, c->codes.as<uint32_t>(),
                              c->regbits.as<uint64_t>(), c->irr.as<int64_t>(), c->nirr.as<unsigned long long>(), s))
        return rc;
    if (n_irr) {
        ROGTK_HIP_CHECK(hipMemcpyAsync(n_irr, c->nirr.p, 8, hipMemcpyDeviceToHost, s));
        ROGTK_HIP_CHECK(hipStreamSynchronize(s));
    }
    return ROGTK_OK;
}

int check_offset_width(int ow) {
    ROGTK_REQUIRE(ow == 4 || ow == 8, ROGTK_E_INVALID, "offset_width must be 4 or 8, got %d", ow);
    return ROGTK_OK;
}

int check_host_col(const HostCol& h) {
    if (int rc = check_offset_width(h.ow)) return rc;
    ROGTK_REQUIRE(h.n >= 0, ROGTK_E_INVALID, "n must be >= 0");
    ROGTK_REQUIRE(h.offsets != nullptr, ROGTK_E_INVALID, "offsets must not be NULL");
    ROGTK_REQUIRE(h.values != nullptr || h.off(h.n) == h.off0(), ROGTK_E_INVALID, "values must not be NULL");
    ROGTK_REQUIRE(h.off0() == 0, ROGTK_E_INVALID,
                  "offsets[0] must be 0 (slice the values buffer instead of the offsets)");
    return ROGTK_OK;
}

int empty_str_result(int64_t n, rogtk_str_result* out) {
    const int64_t words = std::max<int64_t>((n + 63) / 64, 1);
    out->n = n;
    out->offsets = (int64_t*)calloc((size_t)n + 1, 8);
    out->values = (uint8_t*)calloc(1, 1);
    out->validity = (uint8_t*)calloc((size_t)words, 8);
    out->values_len = 0;
    out->null_count = 0;
    ROGTK_REQUIRE(out->offsets && out->values && out->validity, ROGTK_E_INVALID, "out of host memory");
    return ROGTK_OK;
}

int str_result_begin(HostCtx* c, int64_t n, const int64_t* d_offsets, const uint64_t* d_valid, const HostCol* h,
                     rogtk_str_result* out) {
    auto run = [&]() -> int {
        if (int rc = empty_str_result(n, out)) return rc;
        const int64_t words = (n + 63) / 64;
        uint64_t* bits = (uint64_t*)out->validity;
        if (h) {
            for (int64_t i = 0; i <= n; ++i) out->offsets[i] = h->off(i);
        } else if (int rc = c->d2h(out->offsets, d_offsets, (size_t)(n + 1) * 8)) {
            return rc;
        }
        if (d_valid) {
            if (int rc = c->d2h(bits, d_valid, (size_t)words * 8)) return rc;
        } else {
            for (int64_t w = 0; w < words; ++w) bits[w] = n - 64 * w >= 64 ? ~0ull : (1ull << (n - 64 * w)) - 1;
        }
        int64_t valid = 0;  // the rows below n only: a device word may carry bits past them
        for (int64_t w = 0; w < words; ++w)
            valid += __builtin_popcountll(n - 64 * w >= 64 ? bits[w] : bits[w] & ((1ull << (n - 64 * w)) - 1));
        out->null_count = n - valid;
        if (h)
            for (int64_t i = 0; i < n; ++i)
                if (!h->valid(i)) str_result_set_null(out, i);
        return ROGTK_OK;
    };
    const int rc = run();
    if (rc) rogtk_str_result_free(out);
    return rc;
}

int str_result_finish(HostCtx* c, DevBuf& dev, const std::function<int(uint8_t*)>& fill, rogtk_str_result* out) {
    auto run = [&]() -> int {
        const int64_t total = out->offsets[out->n];
        if (total <= 0) return ROGTK_OK;  // begin left one zero byte
        free(out->values);
        out->values = (uint8_t*)malloc((size_t)total);
        ROGTK_REQUIRE(out->values, ROGTK_E_INVALID, "out of host memory for %lld output bytes", (long long)total);
        out->values_len = total;
        if (int rc = dev.ensure((size_t)total)) return rc;
        if (int rc = fill(dev.as<uint8_t>())) return rc;
        return c->d2h(out->values, dev.p, (size_t)total);
    };
    const int rc = run();
    if (rc) rogtk_str_result_free(out);
    return rc;
}

}  // namespace rogtk
