// capi.hip — extern "C" surface of librogtk_hip.so (declared in include/rogtk_hip.h), but for the
// UMI cluster / correct family (umi_api.hip) and the entries that live next to their kernels.
//
// Host-side responsibilities: argument validation, thread-local last-error,
// the glibc-log2 entropy tables (bit-exact with the reference's f64::log2),
// Hamming target encoding and launch-bracketing profiling events. The level-2 (host Arrow
// buffer) entries here stand on the shared layer of level2.h (level2.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "level2.h"

namespace rogtk {

// ------------------------------------------------------------------ errors
static thread_local char t_err[1024] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(t_err, sizeof(t_err), fmt, ap);
    va_end(ap);
}

// --------------------------------------------------------------- profiling
const char* const kKernelNames[K_COUNT_] = {
    "stage",          "score_packed",   "score_rows",    "cluster_mark",
    "cluster_bitmap", "cluster_scan",   "cluster_compact", "cluster_union",
    "cluster_flatten", "cluster_label", "cluster_assign", "cluster_irregular",
    "bam_fields",     "bam_scan",       "bam_fill",      "pack_reads",
    "row_gather",     "kmer_lds",      "cluster_resolve", "kmer_minimizer",
    "k_slice_bucket", "k_slice_mark",  "k_or_partials",  "k_scan_rt",
    "k_local_cc",     "k_hook_g",      "k_jump",         "k_roots_check", "k_word_label",
    "pack_gather",    "kmer_wave"};

namespace {
std::atomic<bool> g_prof{false};
std::atomic<uint32_t> g_prof_mask{~0u};  // kernels bracketed while g_prof is on (bit per KernelId)
std::mutex g_prof_mu;
struct ProfRec {
    KernelId id;
    hipEvent_t a, b;
};
std::vector<ProfRec> g_prof_pending;
double g_prof_ms[K_COUNT_] = {0};
int64_t g_prof_n[K_COUNT_] = {0};
// in-kernel spans: each profiled launch writes (entry, exit) ticks per workgroup into a
// slice of one preallocated device arena; the min/max reductions run only at drain time
// (profile_read_span / reset / a full arena), so a profiled launch adds no allocation,
// no kernel and no stream dependency to the pipeline it measures
constexpr int kSpanSlots = 1 << 14;
constexpr size_t kSpanArenaBytes = size_t(256) << 20;  // ~400 launches of 10M rows
uint64_t* g_span_dev = nullptr;    // kSpanSlots results
uint64_t* g_span_arena = nullptr;  // per-workgroup ticks of the pending launches
size_t g_span_used = 0;            // bytes of the arena handed out
struct SpanRec {
    KernelId id;
    size_t off;  // u64 offset of the launch's ticks in the arena
    int64_t nb;  // workgroups
};
std::vector<SpanRec> g_span_pending;
double g_span_ms[K_COUNT_] = {0};
int64_t g_span_n[K_COUNT_] = {0};
double g_span_tick_ms = 0;  // wall_clock64 period in ms

// one workgroup per pending launch: max(exit) - min(entry) over its workgroups
__global__ void k_span_reduce(const uint64_t* __restrict__ arena, const int64_t* __restrict__ desc,
                              uint64_t* __restrict__ out) {
    __shared__ uint64_t s_lo[256], s_hi[256];
    const uint64_t* t = arena + desc[2 * blockIdx.x];
    const int64_t nb = desc[2 * blockIdx.x + 1];
    uint64_t lo = ~0ull, hi = 0;
    for (int64_t b = threadIdx.x; b < nb; b += blockDim.x) {
        lo = min(lo, t[2 * b]);
        hi = max(hi, t[2 * b + 1]);
    }
    s_lo[threadIdx.x] = lo;
    s_hi[threadIdx.x] = hi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s_lo[threadIdx.x] = min(s_lo[threadIdx.x], s_lo[threadIdx.x + o]);
            s_hi[threadIdx.x] = max(s_hi[threadIdx.x], s_hi[threadIdx.x + o]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = s_hi[0] > s_lo[0] ? s_hi[0] - s_lo[0] : 0;
}

void span_drain_locked() {
    if (g_span_pending.empty() || !g_span_dev) return;
    const size_t n = g_span_pending.size();
    std::vector<int64_t> desc(2 * n);
    for (size_t i = 0; i < n; ++i) {
        desc[2 * i] = (int64_t)g_span_pending[i].off;
        desc[2 * i + 1] = g_span_pending[i].nb;
    }
    std::vector<uint64_t> h(n);
    int64_t* d_desc = nullptr;
    bool ok = hipDeviceSynchronize() == hipSuccess && hipMalloc((void**)&d_desc, desc.size() * 8) == hipSuccess;
    if (ok) {
        ok = hipMemcpy(d_desc, desc.data(), desc.size() * 8, hipMemcpyHostToDevice) == hipSuccess;
        if (ok) {
            hipLaunchKernelGGL(k_span_reduce, dim3((unsigned)n), dim3(256), 0, 0, g_span_arena, d_desc, g_span_dev);
            ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
                 hipMemcpy(h.data(), g_span_dev, n * 8, hipMemcpyDeviceToHost) == hipSuccess;
        }
        (void)hipFree(d_desc);
    }
    if (ok)
        for (size_t i = 0; i < n; ++i) {
            g_span_ms[g_span_pending[i].id] += (double)h[i] * g_span_tick_ms;
            g_span_n[g_span_pending[i].id] += 1;
        }
    g_span_pending.clear();
    g_span_used = 0;
}

// timing events are reused (no create / destroy per profiled launch) and released at
// device scope: a system-scope release would write the L2 back at every bracketed launch
std::vector<hipEvent_t> g_prof_free;

hipEvent_t prof_event_locked() {
    if (!g_prof_free.empty()) {
        hipEvent_t e = g_prof_free.back();
        g_prof_free.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    return hipEventCreateWithFlags(&e, hipEventDisableSystemFence) == hipSuccess ? e : nullptr;
}

void prof_drain_locked() {
    for (auto& r : g_prof_pending) {
        float ms = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            g_prof_ms[r.id] += ms;
            g_prof_n[r.id] += 1;
        }
        g_prof_free.push_back(r.a);
        g_prof_free.push_back(r.b);
    }
    g_prof_pending.clear();
}
}  // namespace

bool profiling_on() { return g_prof.load(std::memory_order_relaxed); }

uint64_t* span_begin(KernelId id, int64_t n_blocks, hipStream_t s) {
    (void)s;
    if (!g_prof.load(std::memory_order_relaxed) || !((g_prof_mask.load(std::memory_order_relaxed) >> id) & 1u))
        return nullptr;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (!g_span_dev) {
        int dev = 0, khz = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0 ||
            hipMalloc((void**)&g_span_dev, kSpanSlots * 8) != hipSuccess) {
            g_span_dev = nullptr;
            return nullptr;
        }
        if (hipMalloc((void**)&g_span_arena, kSpanArenaBytes) != hipSuccess) {
            (void)hipFree(g_span_dev);
            g_span_dev = g_span_arena = nullptr;
            return nullptr;
        }
        g_span_tick_ms = 1.0 / (double)khz;
    }
    const size_t need = (size_t)std::max<int64_t>(n_blocks, 1) * 16;
    if (need > kSpanArenaBytes) return nullptr;  // not timed
    if ((int)g_span_pending.size() >= kSpanSlots || g_span_used + need > kSpanArenaBytes) span_drain_locked();
    uint64_t* t = g_span_arena + g_span_used / 8;
    g_span_used += (need + 255) & ~size_t(255);
    return t;
}

void span_end(KernelId id, uint64_t* tspan, int64_t n_blocks, hipStream_t s) {
    (void)s;
    if (!tspan) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_span_pending.push_back({id, (size_t)(tspan - g_span_arena), std::max<int64_t>(n_blocks, 1)});
}

ProfScope::ProfScope(KernelId id, hipStream_t stream, bool exact) : id_(id), stream_(stream), exact_(exact) {
    if (!g_prof.load(std::memory_order_relaxed) || !((g_prof_mask.load(std::memory_order_relaxed) >> id) & 1u)) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    start_ = prof_event_locked();
    if (!start_) return;
    if (exact_) {  // both events ride on the dispatch packet (hipExtLaunchKernelGGL)
        stop_ = prof_event_locked();
        if (!stop_) {
            g_prof_free.push_back(start_);
            start_ = nullptr;
        }
        return;
    }
    hipEventRecord(start_, stream_);
}

ProfScope::~ProfScope() {
    if (!start_) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    hipEvent_t stop = stop_;
    if (!exact_) {
        stop = prof_event_locked();
        if (!stop) {
            g_prof_free.push_back(start_);
            return;
        }
        hipEventRecord(stop, stream_);
    }
    g_prof_pending.push_back({id_, start_, stop});
}

// ------------------------------------------------------------ entropy LUT
double plogp_host(uint32_t c, uint32_t t) {
    // umi_score.rs:67-68 / :140-141: p = count as f64 / total as f64; p * p.log2()
    const double p = (double)c / (double)t;
    return p * std::log2(p);
}

namespace {
struct DevLut {
    double* dev = nullptr;
    int64_t covered = -1;
};
std::mutex g_lut_mu;
std::map<int, DevLut> g_luts;
}  // namespace

int lut_ensure(int64_t max_total, const double** dev, int64_t* covered) {
    int device = 0;
    ROGTK_HIP_CHECK(hipGetDevice(&device));
    std::lock_guard<std::mutex> lk(g_lut_mu);
    DevLut& L = g_luts[device];
    if (L.covered < max_total) {
        int64_t want = std::max<int64_t>(std::max<int64_t>(max_total, 256), L.covered * 2);
        // 4096 covers every UMI/read-length string; the table is 8.4M doubles (67 MB).
        ROGTK_REQUIRE(max_total <= 4096, ROGTK_E_UNSUPPORTED,
                      "byte path: strings longer than 4096 bytes are not supported");
        want = std::min<int64_t>(want, 4096);
        const int64_t entries = lut_index(want + 1, 0);
        std::vector<double> h((size_t)entries, 0.0);
        for (int64_t t = 1; t <= want; ++t)
            for (int64_t c = 1; c <= t; ++c) h[(size_t)lut_index(t, c)] = plogp_host((uint32_t)c, (uint32_t)t);
        double* d = nullptr;
        ROGTK_HIP_CHECK(hipMalloc(&d, (size_t)entries * sizeof(double)));
        ROGTK_HIP_CHECK(hipMemcpy(d, h.data(), (size_t)entries * sizeof(double), hipMemcpyHostToDevice));
        if (L.dev) {
            ROGTK_HIP_CHECK(hipDeviceSynchronize());
            hipFree(L.dev);
        }
        L.dev = d;
        L.covered = want;
    }
    *dev = L.dev;
    *covered = L.covered;
    return ROGTK_OK;
}

int build_packed_params(int L, PackedParams* p) {
    std::memset(p, 0, sizeof(*p));
    p->L = L;
    for (int c = 1; c <= L; ++c) p->sh[c] = plogp_host((uint32_t)c, (uint32_t)L);
    if (L >= 2)
        for (int c = 1; c <= L - 1; ++c) p->di[c] = plogp_host((uint32_t)c, (uint32_t)(L - 1));
    if (L >= 3) {
        const double denom = (double)std::min(L - 2, 64);  // umi_score.rs:90
        for (int u = 0; u <= kMaxPackedLen; ++u) p->ling[u] = (double)u / denom;
    }
    for (int k = 0; k <= L; ++k) p->frac[k] = (double)k / (double)L;  // :120, :31
    return ROGTK_OK;
}

static size_t utf8_next_host(const uint8_t* s, size_t n, size_t i, uint32_t* cp) {
    const uint8_t c = s[i];
    size_t w = c < 0x80 ? 1 : (c >> 5) == 0x6 ? 2 : (c >> 4) == 0xE ? 3 : 4;
    if (i + w > n) w = n - i;
    uint32_t v = w == 1 ? c : w == 2 ? (c & 0x1Fu) : w == 3 ? (c & 0x0Fu) : (c & 0x07u);
    for (size_t k = 1; k < w; ++k) v = (v << 6) | (s[i + k] & 0x3Fu);
    *cp = v;
    return i + w;
}

void encode_target(const uint8_t* target, int64_t tlen, int L, uint32_t maxd, PackedParams* p) {
    p->max_distance = maxd;
    p->tcode = p->cmplo = p->always_mismatch = 0;
    if (!target) {
        p->ham_mode = 0;
        return;
    }
    if (tlen != L) {  // expressions.rs:1057: seq.len() != target.len() -> u32::MAX / false
        p->ham_mode = 2;
        return;
    }
    p->ham_mode = 1;
    // chars().zip(): a packed row is L ASCII chars; the target may hold fewer chars
    // (multi-byte UTF-8) — only the first min(k, L) positions are compared.
    size_t i = 0;
    int j = 0;
    while (i < (size_t)tlen && j < L) {
        uint32_t cp;
        i = utf8_next_host(target, (size_t)tlen, i, &cp);
        const int sh = 2 * (L - 1 - j);
        const int b = cp == 'A' ? 0 : cp == 'C' ? 1 : cp == 'G' ? 2 : cp == 'T' ? 3 : -1;
        if (b < 0) {
            p->always_mismatch += 1;  // a non-ACGT target char never equals a packed base
        } else {
            p->tcode |= (uint32_t)b << sh;
            p->cmplo |= 1u << sh;
        }
        ++j;
    }
}

}  // namespace rogtk

using namespace rogtk;

namespace {

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

int check_packed_alignment(const uint32_t* codes, const ScoreOut& o, const uint32_t* hd) {
    const void* ps[] = {codes, o.sh, o.ling, o.homo, o.di, o.dust, o.comb, o.longest, hd};
    for (const void* p : ps)
        ROGTK_REQUIRE(!p || aligned16(p), ROGTK_E_INVALID,
                      "packed SoA buffers must be 16-byte aligned (device allocations are)");
    return ROGTK_OK;
}

}  // namespace

namespace rogtk {
namespace detail_attach {
thread_local hipEvent_t t_attached = nullptr;  // rogtk_event_attach_next
thread_local bool t_attach_taken = false;
}  // namespace
void arm_attached_event(hipEvent_t e) {
    detail_attach::t_attached = e;
    detail_attach::t_attach_taken = false;
}
bool attached_event_taken() { return detail_attach::t_attach_taken; }
void set_attached_taken() {
    detail_attach::t_attached = nullptr;
    detail_attach::t_attach_taken = true;
}
hipEvent_t take_attached_event() {
    using namespace detail_attach;
    hipEvent_t e = t_attached;
    if (e) {
        t_attached = nullptr;
        t_attach_taken = true;
    }
    return e;
}
}  // namespace rogtk

extern "C" {

const char* rogtk_version(void) { return "rogtk-amd 0.1.0 (gfx950)"; }

const char* rogtk_last_error(void) { return t_err; }

// Pinned host memory for callers' output (and input) buffers: transfers from / to it
// are direct DMA. Freed blocks are cached by size class (2 MiB multiples, up to 16 GiB
// in all) because pinning fresh pages costs more than the copy it saves.
namespace {
std::mutex g_pin_mu;
std::multimap<size_t, void*> g_pin_free;
std::map<void*, size_t> g_pin_size;
size_t g_pin_cached = 0;
constexpr size_t kPinCacheMax = (size_t)16 << 30;
}  // namespace

int rogtk_host_alloc(size_t bytes, void** out) {
    ROGTK_REQUIRE(out, ROGTK_E_INVALID, "host_alloc: NULL out");
    if (int rc = require_device()) return rc;
    const size_t cls = (std::max<size_t>(bytes, 1) + ((size_t)2 << 20) - 1) / ((size_t)2 << 20) * ((size_t)2 << 20);
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        auto it = g_pin_free.find(cls);
        if (it != g_pin_free.end()) {
            *out = it->second;
            g_pin_cached -= cls;
            g_pin_free.erase(it);
            return ROGTK_OK;
        }
    }
    void* p = nullptr;
    ROGTK_HIP_CHECK(hipHostMalloc(&p, cls, hipHostMallocDefault));
    std::lock_guard<std::mutex> lk(g_pin_mu);
    g_pin_size[p] = cls;
    *out = p;
    return ROGTK_OK;
}

int rogtk_host_free(void* p) {
    if (!p) return ROGTK_OK;
    std::lock_guard<std::mutex> lk(g_pin_mu);
    auto it = g_pin_size.find(p);
    ROGTK_REQUIRE(it != g_pin_size.end(), ROGTK_E_INVALID, "host_free: not a rogtk_host_alloc block");
    const size_t cls = it->second;
    if (g_pin_cached + cls <= kPinCacheMax) {
        g_pin_free.emplace(cls, p);
        g_pin_cached += cls;
    } else {
        g_pin_size.erase(it);
        ROGTK_HIP_CHECK(hipHostFree(p));
    }
    return ROGTK_OK;
}

int rogtk_device_count(int* out) {
    ROGTK_REQUIRE(out, ROGTK_E_INVALID, "out_count is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *out = n;
    return ROGTK_OK;
}

int rogtk_stage_strings(const void* offsets, int offset_width, const uint8_t* values,
                        const uint8_t* validity, int64_t validity_offset, int64_t n, int umi_len,
                        uint32_t* codes, uint64_t* regular_bits, int64_t* irregular_rows,
                        int64_t* n_irregular, void* stream) {
    if (int rc = check_offset_width(offset_width)) return rc;
    ROGTK_REQUIRE(n >= 0, ROGTK_E_INVALID, "n must be >= 0");
    ROGTK_REQUIRE(n == 0 || (offsets && codes && regular_bits && irregular_rows && n_irregular),
                  ROGTK_E_INVALID, "stage: NULL buffer");
    hipStream_t s = as_stream(stream);
    if (n_irregular) ROGTK_HIP_CHECK(hipMemsetAsync(n_irregular, 0, 8, s));
    return launch_stage(offsets, offset_width, values, validity, validity_offset, n, umi_len, codes,
                        regular_bits, irregular_rows, (unsigned long long*)n_irregular, s);
}

int rogtk_umi_score_packed(const uint32_t* codes, const uint64_t* regular_bits, int64_t n,
                           int umi_len, const rogtk_umi_scores* scores, const uint8_t* target,
                           int64_t target_len, uint32_t max_distance, uint32_t* hamming_distance,
                           uint64_t* hamming_within_bits, void* stream) {
    ROGTK_REQUIRE(umi_len >= 1 && umi_len <= kMaxPackedLen, ROGTK_E_UNSUPPORTED,
                  "packed path: umi_len %d outside 1..%d", umi_len, kMaxPackedLen);
    ROGTK_REQUIRE(n >= 0, ROGTK_E_INVALID, "n must be >= 0");
    ROGTK_REQUIRE(n == 0 || codes, ROGTK_E_INVALID, "codes is NULL");
    ROGTK_REQUIRE(target_len >= 0, ROGTK_E_INVALID, "target_len must be >= 0");
    const ScoreOut o = to_score_out(scores);
    if (int rc = check_packed_alignment(codes, o, hamming_distance)) return rc;
    PackedParams p;
    build_packed_params(umi_len, &p);
    encode_target(target, target_len, umi_len, max_distance, &p);
    return launch_score_packed(codes, regular_bits, n, p, o, hamming_distance, hamming_within_bits,
                               as_stream(stream));
}

int rogtk_umi_score_assign_packed(const uint32_t* codes, const uint64_t* regular_bits, int64_t n, int umi_len,
                                  const rogtk_umi_scores* scores, const uint8_t* target, int64_t target_len,
                                  uint32_t max_distance, uint32_t* hamming_distance,
                                  uint64_t* hamming_within_bits, const void* cluster_ws,
                                  int64_t cluster_max_distinct, uint32_t* cluster_id, int deferred,
                                  void* stream) {
    ROGTK_REQUIRE(umi_len >= 1 && umi_len <= kMaxPackedLen, ROGTK_E_UNSUPPORTED,
                  "packed path: umi_len %d outside 1..%d", umi_len, kMaxPackedLen);
    ROGTK_REQUIRE(n >= 0, ROGTK_E_INVALID, "n must be >= 0");
    ROGTK_REQUIRE(n == 0 || (codes && cluster_id), ROGTK_E_INVALID, "codes / cluster_id is NULL");
    ROGTK_REQUIRE(cluster_ws, ROGTK_E_INVALID, "score_assign: cluster_ws is NULL");
    ROGTK_REQUIRE(target_len >= 0, ROGTK_E_INVALID, "target_len must be >= 0");
    ROGTK_REQUIRE(aligned16(codes) && aligned16(cluster_id), ROGTK_E_INVALID,
                  "score_assign: codes/cluster_id must be 16-byte aligned");
    const ScoreOut o = to_score_out(scores);
    if (int rc = check_packed_alignment(codes, o, hamming_distance)) return rc;
    ClusterLayout cl;
    if (int rc = cluster_layout(umi_len, cluster_max_distinct, &cl)) return rc;
    PackedParams p;
    build_packed_params(umi_len, &p);
    encode_target(target, target_len, umi_len, max_distance, &p);
    hipStream_t s = as_stream(stream);
    AssignIn a;
    if (int rc = cluster_assign_prepare(cl, (const uint8_t*)cluster_ws, codes, regular_bits, n, cluster_id, s,
                                        deferred != 0, &a))
        return rc;
    const bool any = any_score(o) || (p.ham_mode && (hamming_distance || hamming_within_bits));
    if (a.out && any)  // one pass: scores, Hamming and ids
        return launch_score_packed(codes, regular_bits, n, p, o, hamming_distance, hamming_within_bits, s, &a);
    if (int rc = launch_score_packed(codes, regular_bits, n, p, o, hamming_distance, hamming_within_bits, s))
        return rc;
    return launch_cluster_assign(cl, (const uint8_t*)cluster_ws, codes, regular_bits, n, cluster_id, s,
                                 deferred != 0);
}

int rogtk_umi_score_rows(const void* offsets, int offset_width, const uint8_t* values,
                         const int64_t* rows, const int64_t* n_rows_dev, int64_t max_rows,
                         int64_t max_len, const rogtk_umi_scores* scores, const uint8_t* target,
                         int64_t target_len, uint32_t max_distance, uint32_t* hamming_distance,
                         uint64_t* hamming_within_bits, void* stream) {
    if (int rc = check_offset_width(offset_width)) return rc;
    ROGTK_REQUIRE(max_rows >= 0 && max_len >= 0 && target_len >= 0, ROGTK_E_INVALID,
                  "score_rows: negative size");
    if (max_rows == 0) return ROGTK_OK;
    ROGTK_REQUIRE(offsets && rows, ROGTK_E_INVALID, "score_rows: NULL offsets/rows");
    const double* lut = nullptr;
    int64_t covered = 0;
    if (int rc = lut_ensure(std::max<int64_t>(max_len, 1), &lut, &covered)) return rc;
    hipStream_t s = as_stream(stream);
    const uint8_t* tdev = nullptr;
    thread_local DevBuf t_target;
    if (target) {
        if (int rc = t_target.ensure((size_t)std::max<int64_t>(target_len, 1))) return rc;
        if (target_len)
            ROGTK_HIP_CHECK(hipMemcpyAsync(t_target.p, target, (size_t)target_len, hipMemcpyHostToDevice, s));
        tdev = t_target.as<uint8_t>();
    }
    return launch_score_rows(offsets, offset_width, values, rows, n_rows_dev, max_rows, lut, covered,
                             to_score_out(scores), tdev, target_len, target ? 1 : 0, max_distance,
                             hamming_distance, hamming_within_bits, s);
}

int rogtk_cluster_workspace_size(int umi_len, int64_t max_distinct, int64_t* bytes) {
    ROGTK_REQUIRE(bytes, ROGTK_E_INVALID, "bytes is NULL");
    ClusterLayout cl;
    if (int rc = cluster_layout(umi_len, max_distinct, &cl)) return rc;
    *bytes = cl.total;
    return ROGTK_OK;
}

int rogtk_cluster_bitmap_words(int umi_len, int64_t* words) {
    ROGTK_REQUIRE(words, ROGTK_E_INVALID, "words is NULL");
    ClusterLayout cl;
    if (int rc = cluster_layout(umi_len, 1, &cl)) return rc;
    *words = cl.words;
    return ROGTK_OK;
}

int rogtk_cluster_init(void* ws, int umi_len, int64_t max_distinct, void* stream) {
    ClusterLayout cl;
    if (int rc = cluster_layout(umi_len, max_distinct, &cl)) return rc;
    ROGTK_REQUIRE(ws, ROGTK_E_INVALID, "ws is NULL");
    cluster_release(ws);  // a reused address must not inherit a stale pending resolve
    ROGTK_HIP_CHECK(hipMemsetAsync(ws, 0, (size_t)cl.total, as_stream(stream)));
    return ROGTK_OK;
}

int rogtk_cluster_mark(const uint32_t* codes, const uint64_t* regular_bits, int64_t n, int umi_len,
                       void* ws, int64_t max_distinct, void* stream) {
    ROGTK_REQUIRE(ws, ROGTK_E_INVALID, "ws is NULL");
    ClusterLayout cl;
    if (int rc = cluster_layout(umi_len, max_distinct, &cl)) return rc;
    ROGTK_REQUIRE(n >= 0 && (n == 0 || codes), ROGTK_E_INVALID, "mark: bad codes/n");
    ROGTK_REQUIRE(aligned16(codes), ROGTK_E_INVALID, "mark: codes must be 16-byte aligned");
    return launch_cluster_mark(codes, regular_bits, n, umi_len, (uint8_t*)ws + cl.off_presence,
                               as_stream(stream));
}

int rogtk_cluster_local_bitmap(void* ws, int umi_len, int64_t max_distinct, uint64_t* bitmap_out,
                               void* stream) {
    ClusterLayout cl;
    if (int rc = cluster_layout(umi_len, max_distinct, &cl)) return rc;
    ROGTK_REQUIRE(ws && bitmap_out, ROGTK_E_INVALID, "ws/bitmap_out is NULL");
    return launch_cluster_local_bitmap(cl, (uint8_t*)ws, bitmap_out, as_stream(stream));
}

int rogtk_cluster_resolve(void* ws, int umi_len, int64_t max_distinct, const uint64_t* bitmaps,
                          int n_bitmaps, int max_distance, void* stream) {
    ClusterLayout cl;
    if (int rc = cluster_layout(umi_len, max_distinct, &cl)) return rc;
    ROGTK_REQUIRE(ws && bitmaps, ROGTK_E_INVALID, "ws/bitmaps is NULL");
    ROGTK_REQUIRE(n_bitmaps >= 1, ROGTK_E_INVALID, "n_bitmaps must be >= 1");
    ROGTK_REQUIRE(max_distance == 0 || max_distance == 1, ROGTK_E_UNSUPPORTED,
                  "max_distance %d: only 0 (exact) and 1 (Hamming<=1 components) are supported",
                  max_distance);
    return launch_cluster_resolve(cl, (uint8_t*)ws, bitmaps, n_bitmaps, max_distance, as_stream(stream));
}

int rogtk_cluster_assign(const void* ws, int umi_len, int64_t max_distinct, const uint32_t* codes,
                         const uint64_t* regular_bits, int64_t n, uint32_t* cluster_id,
                         void* stream) {
    ClusterLayout cl;
    if (int rc = cluster_layout(umi_len, max_distinct, &cl)) return rc;
    ROGTK_REQUIRE(ws && (n == 0 || (codes && cluster_id)), ROGTK_E_INVALID, "assign: NULL buffer");
    ROGTK_REQUIRE(aligned16(codes) && aligned16(cluster_id), ROGTK_E_INVALID,
                  "assign: codes/cluster_id must be 16-byte aligned");
    return launch_cluster_assign(cl, (const uint8_t*)ws, codes, regular_bits, n, cluster_id,
                                 as_stream(stream));
}

int rogtk_cluster_assign_deferred(const void* ws, int umi_len, int64_t max_distinct, const uint32_t* codes,
                                  const uint64_t* regular_bits, int64_t n, uint32_t* cluster_id, void* stream) {
    ClusterLayout cl;
    if (int rc = cluster_layout(umi_len, max_distinct, &cl)) return rc;
    ROGTK_REQUIRE(ws && (n == 0 || (codes && cluster_id)), ROGTK_E_INVALID, "assign: NULL buffer");
    ROGTK_REQUIRE(aligned16(codes) && aligned16(cluster_id), ROGTK_E_INVALID,
                  "assign: codes/cluster_id must be 16-byte aligned");
    return launch_cluster_assign(cl, (const uint8_t*)ws, codes, regular_bits, n, cluster_id, as_stream(stream),
                                 true);
}

int rogtk_cluster_sync(const void* ws, void* stream, int* redone) {
    ROGTK_REQUIRE(ws, ROGTK_E_INVALID, "ws is NULL");
    return cluster_finish(ws, as_stream(stream), redone);
}

int rogtk_cluster_stats(const void* ws, int umi_len, int64_t max_distinct, int64_t* out4,
                        void* stream) {
    ClusterLayout cl;
    if (int rc = cluster_layout(umi_len, max_distinct, &cl)) return rc;
    ROGTK_REQUIRE(ws && out4, ROGTK_E_INVALID, "stats: NULL buffer");
    hipStream_t s = as_stream(stream);
    if (int rc = cluster_finish(ws, s)) return rc;
    ROGTK_HIP_CHECK(hipMemcpyAsync(out4, (const uint8_t*)ws + cl.off_stats, 32, hipMemcpyDeviceToHost, s));
    ROGTK_HIP_CHECK(hipStreamSynchronize(s));
    return ROGTK_OK;
}

int rogtk_cluster_rounds(const void* ws, void* stream, int* rounds) {
    ROGTK_REQUIRE(ws && rounds, ROGTK_E_INVALID, "rounds: NULL buffer");
    return cluster_rounds(ws, as_stream(stream), rounds);
}

int rogtk_cluster_set_spec_rounds(int n) { return cluster_set_spec_rounds(n); }
int rogtk_cluster_set_lookback_polls(int n) { return cluster_set_lookback_polls(n); }
int rogtk_cluster_set_mark_method(int method) { return cluster_set_mark_method(method); }
int rogtk_cluster_mark_bitmap_temp_bytes(int64_t n, int umi_len, int64_t* bytes) {
    ROGTK_REQUIRE(bytes, ROGTK_E_INVALID, "null bytes");
    return cluster_mark_bitmap_temp(n, umi_len, bytes);
}
int rogtk_cluster_mark_bitmap(const uint32_t* codes, const uint64_t* regular_bits, int64_t n, int umi_len,
                              uint64_t* bitmap_out, void* temp, int64_t temp_bytes, void* stream) {
    ROGTK_REQUIRE((codes || n == 0) && bitmap_out, ROGTK_E_INVALID, "null codes / bitmap_out");
    return launch_cluster_mark_bitmap(codes, regular_bits, n, umi_len, bitmap_out, temp, temp_bytes,
                                      as_stream(stream));
}
int rogtk_cluster_mark_bitmap_phase(const uint32_t* codes, const uint64_t* regular_bits, int64_t n, int umi_len,
                                    uint64_t* bitmap_out, void* temp, int64_t temp_bytes, int phase, void* stream) {
    ROGTK_REQUIRE((codes || n == 0) && bitmap_out, ROGTK_E_INVALID, "null codes / bitmap_out");
    return launch_cluster_mark_phase(codes, regular_bits, n, umi_len, bitmap_out, temp, temp_bytes, phase,
                                     as_stream(stream));
}
int rogtk_cluster_release(const void* ws) {
    if (ws) cluster_release(ws);
    return ROGTK_OK;
}

// ----------------------------------------------------------------- level 2
int rogtk_umi_complexity_host(const void* offsets, int offset_width, const uint8_t* values,
                              int64_t values_len, const uint8_t* validity, int64_t validity_offset,
                              int64_t n, const rogtk_umi_scores* out) {
    HostCol h{offsets, offset_width, values, values_len, validity, validity_offset, n};
    if (int rc = check_host_col(h)) return rc;
    ROGTK_REQUIRE(out, ROGTK_E_INVALID, "out is NULL");
    if (n == 0) return ROGTK_OK;
    HostCtx* c;
    if (int rc = host_ctx(&c)) return rc;
    DevCol col;
    if (int rc = upload_col(c, 0, h, &col)) return rc;
    const int L = h.first_len();
    int64_t n_irr = 0;
    if (int rc = stage_uploaded(c, col, L, &n_irr, c->stream)) return rc;
    int64_t max_len = 0;  // only the byte path (irregular rows) needs it
    if (n_irr > 0)
        if (int rc = device_max_len(c, col, &max_len)) return rc;
    const ScoreOut ho = to_score_out(out);
    // device outputs
    double* dptr[6] = {nullptr};
    const double* hptr[6] = {ho.sh, ho.ling, ho.homo, ho.di, ho.dust, ho.comb};
    for (int k = 0; k < 6; ++k)
        if (hptr[k]) {
            if (int rc = c->out[k].ensure((size_t)n * 8)) return rc;
            dptr[k] = c->out[k].as<double>();
        }
    uint32_t* dlong = nullptr;
    if (ho.longest) {
        if (int rc = c->out[6].ensure((size_t)n * 4)) return rc;
        dlong = c->out[6].as<uint32_t>();
    }
    rogtk_umi_scores ds{dptr[0], dptr[1], dptr[2], dptr[3], dlong, dptr[4], dptr[5]};
    const bool packable = L >= 1 && L <= kMaxPackedLen;
    if (packable) {
        int rc = rogtk_umi_score_packed(c->codes.as<uint32_t>(), c->regbits.as<uint64_t>(), n, L, &ds,
                                        nullptr, 0, 0, nullptr, nullptr, c->stream);
        if (rc) return rc;
    }
    if (n_irr > 0) {
        int rc = rogtk_umi_score_rows(col.offsets, col.ow, col.values,
                                      c->irr.as<int64_t>(), nullptr, n_irr, max_len, &ds, nullptr, 0,
                                      0, nullptr, nullptr, c->stream);
        if (rc) return rc;
    }
    for (int k = 0; k < 6; ++k)
        if (hptr[k])
            if (int rc = c->d2h((void*)hptr[k], dptr[k], (size_t)n * 8)) return rc;
    if (ho.longest)
        if (int rc = c->d2h(ho.longest, dlong, (size_t)n * 4)) return rc;
    return ROGTK_OK;
}

int rogtk_hamming_host(const void* offsets, int offset_width, const uint8_t* values,
                       int64_t values_len, const uint8_t* validity, int64_t validity_offset,
                       int64_t n, const uint8_t* target, int64_t target_len, uint32_t max_distance,
                       uint32_t* distance, uint8_t* within_bits) {
    HostCol h{offsets, offset_width, values, values_len, validity, validity_offset, n};
    if (int rc = check_host_col(h)) return rc;
    ROGTK_REQUIRE(target || target_len == 0, ROGTK_E_INVALID, "target is NULL");
    ROGTK_REQUIRE(target_len >= 0, ROGTK_E_INVALID, "target_len must be >= 0");
    if (n == 0) return ROGTK_OK;
    static const uint8_t kEmpty = 0;
    const uint8_t* tg = target ? target : &kEmpty;
    HostCtx* c;
    if (int rc = host_ctx(&c)) return rc;
    DevCol col;
    if (int rc = upload_col(c, 0, h, &col)) return rc;
    const int L = h.first_len();
    int64_t n_irr = 0;
    if (int rc = stage_uploaded(c, col, L, &n_irr, c->stream)) return rc;
    int64_t max_len = 0;  // only the byte path (irregular rows) needs it
    if (n_irr > 0)
        if (int rc = device_max_len(c, col, &max_len)) return rc;
    uint32_t* dd = nullptr;
    uint64_t* dw = nullptr;
    if (distance) {
        if (int rc = c->out[0].ensure((size_t)n * 4)) return rc;
        dd = c->out[0].as<uint32_t>();
    }
    const int64_t words = (n + 63) / 64;
    if (within_bits) {
        if (int rc = c->out[1].ensure((size_t)words * 8)) return rc;
        dw = c->out[1].as<uint64_t>();
    }
    if (L >= 1 && L <= kMaxPackedLen) {
        int rc = rogtk_umi_score_packed(c->codes.as<uint32_t>(), c->regbits.as<uint64_t>(), n, L,
                                        nullptr, tg, target_len, max_distance, dd, dw, c->stream);
        if (rc) return rc;
    } else if (dw) {
        ROGTK_HIP_CHECK(hipMemsetAsync(dw, 0, (size_t)words * 8, c->stream));
    }
    if (n_irr > 0) {
        int rc = rogtk_umi_score_rows(col.offsets, col.ow, col.values,
                                      c->irr.as<int64_t>(), nullptr, n_irr, max_len, nullptr, tg,
                                      target_len, max_distance, dd, dw, c->stream);
        if (rc) return rc;
    }
    if (distance)
        if (int rc = c->d2h(distance, dd, (size_t)n * 4)) return rc;
    if (within_bits)
        if (int rc = c->d2h(within_bits, dw, (size_t)(n + 7) / 8)) return rc;
    return ROGTK_OK;
}

// ------------------------------------ cell-barcode correction (barcode.hip)
int rogtk_barcode_set_probe(int probe) { return barcode_set_probe(probe); }

int rogtk_barcode_whitelist_create(const rogtk_str_col* wl, void** out) {
    ROGTK_REQUIRE(wl && out, ROGTK_E_INVALID, "barcode whitelist: NULL argument");
    *out = nullptr;
    const HostCol h(*wl);
    if (int rc = check_host_col(h)) return rc;
    const int64_t W = h.n;
    ROGTK_REQUIRE(W >= 1, ROGTK_E_INVALID, "barcode whitelist: empty");
    ROGTK_REQUIRE(W < (1ll << 32) - 1, ROGTK_E_INVALID, "barcode whitelist: %lld rows, at most 2^32 - 2", (long long)W);
    ROGTK_REQUIRE(h.valid(0), ROGTK_E_INVALID, "barcode whitelist: row 0 is null");
    const int64_t L = h.off(1) - h.off(0);
    ROGTK_REQUIRE(L >= 1 && L <= 32, ROGTK_E_INVALID, "barcode whitelist: row 0 has %lld bytes, outside 1..32",
                  (long long)L);
    std::vector<uint64_t> codes((size_t)W);
    for (int64_t i = 0; i < W; ++i) {
        ROGTK_REQUIRE(h.valid(i), ROGTK_E_INVALID, "barcode whitelist: row %lld is null", (long long)i);
        ROGTK_REQUIRE(h.off(i + 1) - h.off(i) == L, ROGTK_E_INVALID,
                      "barcode whitelist: row %lld has %lld bytes, row 0 has %lld", (long long)i,
                      (long long)(h.off(i + 1) - h.off(i)), (long long)L);
        uint64_t c = 0;
        for (int64_t j = 0; j < L; ++j) {
            const uint8_t ch = h.values[h.off(i) + j];
            const int b = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : -1;
            ROGTK_REQUIRE(b >= 0, ROGTK_E_INVALID, "barcode whitelist: row %lld has byte 0x%02x at position %lld (only ACGT)",
                          (long long)i, ch, (long long)j);
            c = (c << 2) | (uint64_t)b;
        }
        codes[(size_t)i] = c;
    }
    HostCtx* c;
    if (int rc = host_ctx(&c)) return rc;
    return barcode_whitelist_build(codes.data(), W, (int)L, out, c->stream);
}

void rogtk_barcode_whitelist_free(void* handle) { barcode_whitelist_free(handle); }

int rogtk_barcode_whitelist_info(const void* handle, int64_t* W, int* L, int* prefix_digits, int64_t* device_bytes) {
    return barcode_whitelist_info(handle, W, L, prefix_digits, device_bytes);
}

namespace {

static int check_barcode(const char* name, const void* handle, int64_t n, int ambiguous, int64_t* W) {
    ROGTK_REQUIRE(handle, ROGTK_E_INVALID, "%s: NULL whitelist handle", name);
    ROGTK_REQUIRE(n >= 0 && n < (1ll << 31), ROGTK_E_UNSUPPORTED, "%s: n %lld outside 0..2^31-1", name, (long long)n);
    ROGTK_REQUIRE(ambiguous == ROGTK_BC_COUNTS || ambiguous == ROGTK_BC_REJECT, ROGTK_E_INVALID,
                  "%s: ambiguous %d is neither 0 (counts) nor 1 (reject)", name, ambiguous);
    return barcode_whitelist_info(handle, W, nullptr, nullptr, nullptr);
}

}  // namespace

int rogtk_barcode_correct_dev(const void* handle, const int64_t* offsets, const uint8_t* values,
                              const uint8_t* validity, int64_t n, int ambiguous, const uint32_t* prior_counts,
                              uint32_t* index, uint8_t* status, uint32_t* exact_counts, uint32_t* counts,
                              int64_t* totals5, void* stream) {
    int64_t W = 0;
    if (int rc = check_barcode("barcode_correct_dev", handle, n, ambiguous, &W)) return rc;
    ROGTK_REQUIRE(n == 0 || (offsets && values && index && status), ROGTK_E_INVALID,
                  "barcode_correct_dev: NULL argument");
    static uint32_t no_index;  // an empty column still runs the correcting path
    static uint8_t no_status;
    return barcode_correct(handle, DevCol(offsets, values, validity, n), ambiguous, prior_counts,
                           index ? index : &no_index, status ? status : &no_status, exact_counts, counts, false,
                           totals5, as_stream(stream));
}

int rogtk_barcode_count_dev(const void* handle, const int64_t* offsets, const uint8_t* values,
                            const uint8_t* validity, int64_t n, uint32_t* exact_counts, int64_t* totals5,
                            void* stream) {
    int64_t W = 0;
    if (int rc = check_barcode("barcode_count_dev", handle, n, ROGTK_BC_COUNTS, &W)) return rc;
    ROGTK_REQUIRE(exact_counts && (n == 0 || (offsets && values)), ROGTK_E_INVALID, "barcode_count_dev: NULL argument");
    return barcode_correct(handle, DevCol(offsets, values, validity, n), ROGTK_BC_COUNTS, nullptr, nullptr, nullptr,
                           exact_counts, nullptr, true, totals5, as_stream(stream));
}

int rogtk_barcode_count_host(const void* handle, const rogtk_str_col* col, uint32_t* exact_counts, int64_t* totals5) {
    ROGTK_REQUIRE(col && exact_counts, ROGTK_E_INVALID, "barcode_count: NULL argument");
    int64_t W = 0;
    if (int rc = check_barcode("barcode_count", handle, col->n, ROGTK_BC_COUNTS, &W)) return rc;
    const HostCol h(*col);
    if (int rc = check_host_col(h)) return rc;
    HostCtx* c;
    if (int rc = host_ctx(&c)) return rc;
    DevCol dcol;
    if (int rc = upload_col(c, 0, h, &dcol)) return rc;
    if (int rc = c->out[1].ensure((size_t)W * 4)) return rc;
    if (int rc = c->h2d(c->out[1].p, exact_counts, (size_t)W * 4)) return rc;
    if (int rc = barcode_correct(handle, dcol, ROGTK_BC_COUNTS, nullptr, nullptr, nullptr,
                                 c->out[1].as<uint32_t>(), nullptr, true, totals5, c->stream))
        return rc;
    return c->d2h(exact_counts, c->out[1].p, (size_t)W * 4);
}

int rogtk_barcode_correct_host(const void* handle, const rogtk_str_col* col, int ambiguous,
                               const uint32_t* prior_counts, uint32_t* index, uint8_t* status,
                               rogtk_str_result* corrected, uint32_t* exact_counts, uint32_t* counts,
                               int64_t* totals5) {
    if (corrected) *corrected = rogtk_str_result{};
    ROGTK_REQUIRE(col, ROGTK_E_INVALID, "barcode_correct: NULL column");
    int64_t W = 0;
    if (int rc = check_barcode("barcode_correct", handle, col->n, ambiguous, &W)) return rc;
    const HostCol h(*col);
    if (int rc = check_host_col(h)) return rc;
    const int64_t n = h.n;
    ROGTK_REQUIRE(n == 0 || (index && status), ROGTK_E_INVALID, "barcode_correct: index or status is NULL");
    HostCtx* c;
    if (int rc = host_ctx(&c)) return rc;
    auto run = [&]() -> int {
        DevCol dcol;
        if (int rc = upload_col(c, 0, h, &dcol)) return rc;
        const int64_t n1 = std::max<int64_t>(n, 1);
        if (c->out[0].ensure((size_t)n1 * 4) || c->out[1].ensure((size_t)W * 4) || c->out[2].ensure((size_t)W * 4) ||
            c->out[3].ensure((size_t)W * 4) || c->out[7].ensure((size_t)n1))
            return ROGTK_E_HIP;
        uint32_t* d_index = c->out[0].as<uint32_t>();
        uint8_t* d_status = c->out[7].as<uint8_t>();
        if (prior_counts)
            if (int rc = c->h2d(c->out[3].p, prior_counts, (size_t)W * 4)) return rc;
        if (int rc = barcode_correct(handle, dcol, ambiguous, prior_counts ? c->out[3].as<uint32_t>() : nullptr,
                                     d_index, d_status,
                                     c->out[1].as<uint32_t>(), c->out[2].as<uint32_t>(), false, totals5, c->stream))
            return rc;
        if (n > 0) {
            if (int rc = c->d2h(index, d_index, (size_t)n * 4)) return rc;
            if (int rc = c->d2h(status, d_status, (size_t)n)) return rc;
        }
        if (exact_counts)
            if (int rc = c->d2h(exact_counts, c->out[1].p, (size_t)W * 4)) return rc;
        if (counts)
            if (int rc = c->d2h(counts, c->out[2].p, (size_t)W * 4)) return rc;
        if (!corrected) return ROGTK_OK;
        if (n == 0) return empty_str_result(0, corrected);
        int64_t tb = 0;
        if (int rc = barcode_corrected_temp(n, &tb)) return rc;
        if (c->out[4].ensure((size_t)(n + 1) * 8) || c->out[5].ensure((size_t)tb)) return ROGTK_E_HIP;
        if (int rc = barcode_corrected_measure(handle, d_status, n, c->out[4].as<int64_t>(), c->out[5].p, tb,
                                               c->stream))
            return rc;
        if (int rc = str_result_begin(c, n, c->out[4].as<int64_t>(), nullptr, nullptr, corrected)) return rc;
        for (int64_t i = 0; i < n; ++i)
            if (status[i] > ROGTK_BC_CORRECTED) str_result_set_null(corrected, i);
        return str_result_finish(
            c, c->out[6],
            [&](uint8_t* d) {
                return barcode_corrected_fill(handle, d_index, d_status, n, c->out[4].as<int64_t>(), d, c->stream);
            },
            corrected);
    };
    const int rc = run();
    if (rc && corrected) rogtk_str_result_free(corrected);
    return rc;
}

// --------------------------------------------------------------- stream events
int rogtk_event_create(int flags, void** out) {
    ROGTK_REQUIRE(out, ROGTK_E_INVALID, "event_create: NULL out");
    *out = nullptr;
    ROGTK_REQUIRE((flags & ~1) == 0, ROGTK_E_INVALID, "event_create: unknown flags %d", flags);
    hipEvent_t e = nullptr;
    const unsigned f = hipEventDisableTiming | ((flags & 1) ? hipEventDisableSystemFence : 0u);
    ROGTK_HIP_CHECK(hipEventCreateWithFlags(&e, f));
    *out = e;
    return ROGTK_OK;
}

int rogtk_event_destroy(void* ev) {
    if (!ev) return ROGTK_OK;
    ROGTK_HIP_CHECK(hipEventDestroy((hipEvent_t)ev));
    return ROGTK_OK;
}

int rogtk_event_attach_next(void* ev) {
    rogtk::detail_attach::t_attached = (hipEvent_t)ev;
    rogtk::detail_attach::t_attach_taken = false;
    return ROGTK_OK;
}

int rogtk_event_attach_done(int* taken) {
    ROGTK_REQUIRE(taken, ROGTK_E_INVALID, "event_attach_done: NULL argument");
    *taken = rogtk::detail_attach::t_attach_taken ? 1 : 0;
    rogtk::detail_attach::t_attached = nullptr;
    rogtk::detail_attach::t_attach_taken = false;
    return ROGTK_OK;
}

int rogtk_event_record(void* ev, void* stream) {
    ROGTK_REQUIRE(ev, ROGTK_E_INVALID, "event_record: NULL event");
    ROGTK_HIP_CHECK(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
    return ROGTK_OK;
}

int rogtk_stream_wait_event(void* stream, void* ev) {
    ROGTK_REQUIRE(ev, ROGTK_E_INVALID, "stream_wait_event: NULL event");
    ROGTK_HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev, 0));
    return ROGTK_OK;
}

int rogtk_event_query(void* ev, int* done) {
    ROGTK_REQUIRE(ev && done, ROGTK_E_INVALID, "event_query: NULL argument");
    const hipError_t e = hipEventQuery((hipEvent_t)ev);
    if (e == hipErrorNotReady) {
        (void)hipGetLastError();
        *done = 0;
        return ROGTK_OK;
    }
    ROGTK_HIP_CHECK(e);
    *done = 1;
    return ROGTK_OK;
}

int rogtk_event_synchronize(void* ev) {
    ROGTK_REQUIRE(ev, ROGTK_E_INVALID, "event_synchronize: NULL event");
    ROGTK_HIP_CHECK(hipEventSynchronize((hipEvent_t)ev));
    return ROGTK_OK;
}

// --------------------------------------------------------------- profiling
int rogtk_profile_enable(int on) {
    g_prof.store(on != 0);
    return ROGTK_OK;
}

int rogtk_profile_select(const char* kernel) {
    if (!kernel || !kernel[0]) {
        g_prof_mask.store(~0u);
        return ROGTK_OK;
    }
    // one name or a comma-separated list
    uint32_t mask = 0;
    for (const char* p = kernel; *p;) {
        const char* e = std::strchr(p, ',');
        const size_t len = e ? (size_t)(e - p) : std::strlen(p);
        int found = -1;
        for (int k = 0; k < K_COUNT_; ++k)
            if (std::strlen(kKernelNames[k]) == len && std::strncmp(p, kKernelNames[k], len) == 0) found = k;
        if (found < 0) {
            set_error("profile_select: unknown kernel '%.*s'", (int)len, p);
            return ROGTK_E_INVALID;
        }
        mask |= 1u << found;
        p += len + (e ? 1 : 0);
    }
    g_prof_mask.store(mask);
    return ROGTK_OK;
}

int rogtk_profile_reset(void) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    prof_drain_locked();
    span_drain_locked();
    for (int k = 0; k < K_COUNT_; ++k) {
        g_prof_ms[k] = 0;
        g_prof_n[k] = 0;
        g_span_ms[k] = 0;
        g_span_n[k] = 0;
    }
    return ROGTK_OK;
}

int rogtk_profile_read_span(const char* kernel, double* total_ms, int64_t* launches) {
    ROGTK_REQUIRE(kernel && total_ms && launches, ROGTK_E_INVALID, "profile_read_span: NULL argument");
    std::lock_guard<std::mutex> lk(g_prof_mu);
    span_drain_locked();
    for (int k = 0; k < K_COUNT_; ++k)
        if (std::strcmp(kernel, kKernelNames[k]) == 0) {
            *total_ms = g_span_ms[k];
            *launches = g_span_n[k];
            return ROGTK_OK;
        }
    set_error("profile_read_span: unknown kernel '%s'", kernel);
    return ROGTK_E_INVALID;
}

int rogtk_profile_read(const char* kernel, double* total_ms, int64_t* launches) {
    ROGTK_REQUIRE(kernel && total_ms && launches, ROGTK_E_INVALID, "profile_read: NULL argument");
    std::lock_guard<std::mutex> lk(g_prof_mu);
    prof_drain_locked();
    for (int k = 0; k < K_COUNT_; ++k)
        if (std::strcmp(kernel, kKernelNames[k]) == 0) {
            *total_ms = g_prof_ms[k];
            *launches = g_prof_n[k];
            return ROGTK_OK;
        }
    set_error("profile_read: unknown kernel '%s'", kernel);
    return ROGTK_E_INVALID;
}

}  // extern "C"
