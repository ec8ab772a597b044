// strings.hip — element-wise DNA / CIGAR / PHRED string transforms on gfx950
// (the remaining per-row string expressions of rogtk).
//
//   op                         reference (src/expressions.rs)
//   ROGTK_STR_REVCOMP          reverse_complement_series / _to_output   :957-977
//   ROGTK_STR_PARSE_CIGAR      parse_cigar_series / parse_cigar_str     :450-505
//   ROGTK_STR_ALIGNED_REF      cigar_aligned_ref_expr + expand_cigar_   :257-394
//   ROGTK_STR_ALIGNED_QUERY    cigar_aligned_query_expr   alignment     :257-336,396-444
//   ROGTK_STR_CIGAR_INSERTIONS extract_cigar_insertions_expr            :29-80,207-251
//   ROGTK_STR_ENRICH_ALLELE    enrich_allele_insertions_expr            :84-205
//   ROGTK_STR_PHRED_STR        phred_to_numeric_series_str / split_string :632-665
//   ROGTK_STR_PHRED_LIST       phred_to_numeric_series (List[u8] values) :598-630
//
// Every op is ONE function (strings_rows.h, shared with a host harness) run twice
// over the rows (thread per row): a measuring pass that only counts output bytes,
// then, after an exclusive scan of the counts, a filling pass that writes them at the
// row's offset. The emitter is the only difference between the passes, so the two can
// never disagree. The per-row cap (ROGTK_STR_MAX_ROW_BYTES) and the insertion bounds
// live in that header; this file holds the column layout, the kernels and the ABI.
#include <hipcub/hipcub.hpp>

#include <cstdlib>
#include <memory>
#include <vector>

#include "rogtk_internal.h"
#include "strings_rows.h"

namespace rogtk {
namespace {

using namespace str_rows;

constexpr int kBlock = 256;

struct Col {
    const void* off;
    int ow;
    const uint8_t* val;
    const uint8_t* valid;
    int64_t voff;
    int bcast;  // row 0 for every row (a length-1 column broadcast)
};

struct Cols {
    Col c[3];
};

__device__ __forceinline__ int64_t col_off(const Col& c, int64_t i) {
    return c.ow == 4 ? (int64_t)((const int32_t*)c.off)[i] : ((const int64_t*)c.off)[i];
}
__device__ __forceinline__ bool col_valid(const Col& c, int64_t i) {
    if (c.bcast) i = 0;
    if (!c.valid) return true;
    const int64_t b = c.voff + i;
    return (c.valid[b >> 3] >> (b & 7)) & 1;
}

__device__ __forceinline__ Str col_str(const Col& c, int64_t i) {
    if (c.bcast) i = 0;
    const int64_t a = col_off(c, i), b = col_off(c, i + 1);
    return Str{c.val + a, (uint64_t)(b - a)};
}

struct OpArgs {
    int op;
    int64_t n;
    int64_t param;
    Cols cols;
};

// "row i of column k" of the device columns, for run_row (strings_rows.h)
struct DevRows {
    const Col* c;
    __device__ __forceinline__ bool valid(int k, int64_t i) const { return col_valid(c[k], i); }
    __device__ __forceinline__ Str str(int k, int64_t i) const { return col_str(c[k], i); }
};

// lengths[i] = output bytes of row i (0 for null rows; ROGTK_STR_MAX_ROW_BYTES + 1 for a
// row over the cap, which stays valid); validity bit per row (ballot)
__global__ __launch_bounds__(kBlock) void k_str_measure(OpArgs a, int64_t* __restrict__ lengths,
                                                        uint64_t* __restrict__ valid_bits) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool ok = false;
    if (i < a.n) {
        Emit<false> o{nullptr};
        ok = run_row(a.op, a.param, DevRows{a.cols.c}, i, o);
        lengths[i] = ok ? (int64_t)o.n : 0;
    }
    const uint64_t m = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && i < a.n) valid_bits[i >> 6] = m;
}

// nothing is written for a row that measured over the cap
__global__ __launch_bounds__(kBlock) void k_str_fill(OpArgs a, const int64_t* __restrict__ offsets,
                                                     uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const int64_t at = offsets[i];
    if (offsets[i + 1] - at > (int64_t)kRowCap) return;
    Emit<true> o{out + at};
    run_row(a.op, a.param, DevRows{a.cols.c}, i, o);
}

int n_inputs(int op) {
    switch (op) {
        case ROGTK_STR_REVCOMP:
        case ROGTK_STR_PARSE_CIGAR:
        case ROGTK_STR_PHRED_STR:
        case ROGTK_STR_PHRED_LIST:
            return 1;
        case ROGTK_STR_CIGAR_INSERTIONS:
            return 2;
        case ROGTK_STR_ALIGNED_REF:
        case ROGTK_STR_ALIGNED_QUERY:
        case ROGTK_STR_ENRICH_ALLELE:
            return 3;
        default:
            return -1;
    }
}

int make_args(int op, const rogtk_str_col* cols, int n_cols, int64_t n_rows, int64_t param, OpArgs* a) {
    const int need = n_inputs(op);
    ROGTK_REQUIRE(need > 0, ROGTK_E_INVALID, "unknown string op %d", op);
    ROGTK_REQUIRE(n_cols == need, ROGTK_E_INVALID, "string op %d takes %d input columns, got %d", op, need, n_cols);
    ROGTK_REQUIRE(n_rows >= 0, ROGTK_E_INVALID, "n_rows must be >= 0");
    if (op == ROGTK_STR_PARSE_CIGAR) param = param != 0;
    if (op == ROGTK_STR_PHRED_STR || op == ROGTK_STR_PHRED_LIST)
        ROGTK_REQUIRE(param >= 0 && param <= 255, ROGTK_E_INVALID, "base %lld does not fit in u8", (long long)param);
    *a = OpArgs{op, n_rows, param, {}};
    for (int k = 0; k < need; ++k) {
        const rogtk_str_col& c = cols[k];
        ROGTK_REQUIRE(c.offset_width == 4 || c.offset_width == 8, ROGTK_E_INVALID, "offset_width must be 4 or 8");
        ROGTK_REQUIRE(c.n == n_rows || c.n == 1, ROGTK_E_INVALID,
                      "input %d has %lld rows (expected %lld or a broadcast of 1)", k, (long long)c.n,
                      (long long)n_rows);
        a->cols.c[k] = Col{c.offsets, c.offset_width, c.values, c.validity, c.validity_offset,
                           c.n == 1 && n_rows != 1 ? 1 : 0};
    }
    return ROGTK_OK;
}

inline unsigned grid_rows(int64_t n) { return (unsigned)std::max<int64_t>((n + kBlock - 1) / kBlock, 1); }

// per-thread scan scratch of the host entry point
struct StrCtx {
    int device = -1;
    hipStream_t stream = nullptr;
    DevBuf off[3], val[3], valid[3], lengths, offsets, bits, cub, out;
    ~StrCtx() {
        if (stream) hipStreamDestroy(stream);
    }
};
thread_local std::unique_ptr<StrCtx> t_str;

}  // namespace
}  // namespace rogtk

using namespace rogtk;

extern "C" {

int rogtk_str_temp_bytes(int64_t n_rows, int64_t* bytes) {
    ROGTK_REQUIRE(bytes && n_rows >= 0, ROGTK_E_INVALID, "bad arguments");
    size_t tb = 0;
    ROGTK_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (const int64_t*)nullptr, (int64_t*)nullptr,
                                                     (int)(n_rows + 1)));
    // lengths (n + 1 int64, padded to 256 B) + the scan's own storage: exactly what
    // measure asks for, so one byte less is an error there
    *bytes = (int64_t)(((size_t)(n_rows + 1) * 8 + 255) / 256 * 256 + tb);
    return ROGTK_OK;
}

int rogtk_str_measure(int op, const rogtk_str_col* cols, int n_cols, int64_t n_rows, int64_t param,
                      int64_t* out_offsets, uint64_t* out_valid_bits, void* temp, int64_t temp_bytes,
                      void* stream) {
    OpArgs a;
    if (int rc = make_args(op, cols, n_cols, n_rows, param, &a)) return rc;
    ROGTK_REQUIRE(n_rows < (int64_t)1 << 31, ROGTK_E_UNSUPPORTED, "at most 2^31 - 1 rows per call");
    ROGTK_REQUIRE(out_offsets && out_valid_bits && temp, ROGTK_E_INVALID, "null output / temp pointer");
    hipStream_t s = (hipStream_t)stream;
    int64_t* lengths = (int64_t*)temp;
    const size_t head = ((size_t)(n_rows + 1) * 8 + 255) / 256 * 256;
    size_t tb = 0;
    ROGTK_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, lengths, out_offsets, (int)(n_rows + 1), s));
    ROGTK_REQUIRE((int64_t)(head + tb) <= temp_bytes, ROGTK_E_INVALID, "temp_bytes %lld too small (need %lld)",
                  (long long)temp_bytes, (long long)(head + tb));
    ROGTK_HIP_CHECK(hipMemsetAsync(lengths + n_rows, 0, 8, s));
    if (n_rows > 0)
        hipLaunchKernelGGL(k_str_measure, dim3(grid_rows(n_rows)), dim3(kBlock), 0, s, a, lengths, out_valid_bits);
    ROGTK_HIP_CHECK(hipGetLastError());
    ROGTK_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum((uint8_t*)temp + head, tb, lengths, out_offsets,
                                                     (int)(n_rows + 1), s));
    return ROGTK_OK;
}

int rogtk_str_fill(int op, const rogtk_str_col* cols, int n_cols, int64_t n_rows, int64_t param,
                   const int64_t* offsets, uint8_t* out_values, void* stream) {
    OpArgs a;
    if (int rc = make_args(op, cols, n_cols, n_rows, param, &a)) return rc;
    if (n_rows > 0)
        hipLaunchKernelGGL(k_str_fill, dim3(grid_rows(n_rows)), dim3(kBlock), 0, (hipStream_t)stream, a, offsets,
                           out_values);
    ROGTK_HIP_CHECK(hipGetLastError());
    return ROGTK_OK;
}

int rogtk_str_transform_host(int op, const rogtk_str_col* cols, int n_cols, int64_t n_rows, int64_t param,
                             rogtk_str_result* out) {
    ROGTK_REQUIRE(out && cols, ROGTK_E_INVALID, "null argument");
    *out = rogtk_str_result{};
    {
        OpArgs chk;
        if (int rc = make_args(op, cols, n_cols, n_rows, param, &chk)) return rc;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available (librogtk_hip needs an MI355X / gfx950 GPU)");
        return ROGTK_E_NODEVICE;
    }
    int dev = 0;
    ROGTK_HIP_CHECK(hipGetDevice(&dev));
    if (!t_str || t_str->device != dev) {
        t_str.reset(new StrCtx());
        t_str->device = dev;
        ROGTK_HIP_CHECK(hipStreamCreateWithFlags(&t_str->stream, hipStreamNonBlocking));
    }
    StrCtx* c = t_str.get();
    hipStream_t s = c->stream;
    // upload the input columns (values [off(0), off(n)); offsets rebased to 0)
    rogtk_str_col dcols[3];
    std::vector<int64_t> off64;
    for (int k = 0; k < n_cols; ++k) {
        const rogtk_str_col& h = cols[k];
        const int64_t n = h.n;
        off64.resize(n + 1);
        for (int64_t r = 0; r <= n; ++r)
            off64[r] = h.offset_width == 4 ? ((const int32_t*)h.offsets)[r] : ((const int64_t*)h.offsets)[r];
        const int64_t base = off64[0], vb = off64[n] - base;
        ROGTK_REQUIRE(vb >= 0 && (h.values_len < 0 || off64[n] <= h.values_len), ROGTK_E_INVALID,
                      "input %d: offsets reference bytes outside values", k);
        for (int64_t r = 0; r <= n; ++r) off64[r] -= base;
        if (c->off[k].ensure((size_t)(n + 1) * 8) || c->val[k].ensure((size_t)std::max<int64_t>(vb, 1)))
            return ROGTK_E_HIP;
        ROGTK_HIP_CHECK(hipMemcpyAsync(c->off[k].p, off64.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, s));
        if (vb > 0)
            ROGTK_HIP_CHECK(hipMemcpyAsync(c->val[k].p, h.values + base, (size_t)vb, hipMemcpyHostToDevice, s));
        const uint8_t* dvalid = nullptr;
        if (h.validity) {
            const size_t nb = (size_t)((h.validity_offset + n + 7) / 8);
            if (c->valid[k].ensure(std::max<size_t>(nb, 1))) return ROGTK_E_HIP;
            ROGTK_HIP_CHECK(hipMemcpyAsync(c->valid[k].p, h.validity, nb, hipMemcpyHostToDevice, s));
            dvalid = c->valid[k].as<uint8_t>();
        }
        // the host staging buffer is reused by the next column: wait for the copy
        ROGTK_HIP_CHECK(hipStreamSynchronize(s));
        dcols[k] = rogtk_str_col{c->off[k].p, 8, c->val[k].as<uint8_t>(), vb, dvalid, h.validity_offset, n};
    }
    int64_t tb = 0;
    if (int rc = rogtk_str_temp_bytes(n_rows, &tb)) return rc;
    const int64_t words = std::max<int64_t>((n_rows + 63) / 64, 1);
    if (c->cub.ensure((size_t)tb) || c->offsets.ensure((size_t)(n_rows + 1) * 8) ||
        c->bits.ensure((size_t)words * 8))
        return ROGTK_E_HIP;
    if (int rc = rogtk_str_measure(op, dcols, n_cols, n_rows, param, c->offsets.as<int64_t>(), c->bits.as<uint64_t>(),
                                   c->cub.p, tb, s))
        return rc;
    int64_t* offs = (int64_t*)malloc((size_t)(n_rows + 1) * 8);
    uint8_t* bits = (uint8_t*)malloc((size_t)words * 8);
    if (!offs || !bits) {
        free(offs);
        free(bits);
        set_error("out of host memory");
        return ROGTK_E_INVALID;
    }
    *out = rogtk_str_result{n_rows, offs, nullptr, 0, bits, 0};
    ROGTK_HIP_CHECK(hipMemcpyAsync(offs, c->offsets.p, (size_t)(n_rows + 1) * 8, hipMemcpyDeviceToHost, s));
    ROGTK_HIP_CHECK(hipMemcpyAsync(bits, c->bits.p, (size_t)words * 8, hipMemcpyDeviceToHost, s));
    ROGTK_HIP_CHECK(hipStreamSynchronize(s));
    // a row over the cap (a CIGAR number far beyond its sequences): an error before the
    // output is allocated or filled
    for (int64_t r = 0; r < n_rows; ++r)
        if (offs[r + 1] - offs[r] > ROGTK_STR_MAX_ROW_BYTES) {
            rogtk_str_result_free(out);
            set_error("row %lld: the output is longer than ROGTK_STR_MAX_ROW_BYTES (%lld bytes)", (long long)r,
                      (long long)ROGTK_STR_MAX_ROW_BYTES);
            return ROGTK_E_UNSUPPORTED;
        }
    const int64_t total = offs[n_rows];
    out->values = (uint8_t*)malloc((size_t)std::max<int64_t>(total, 1));
    ROGTK_REQUIRE(out->values, ROGTK_E_INVALID, "out of host memory for %lld output bytes", (long long)total);
    out->values_len = total;
    if (total > 0) {
        if (c->out.ensure((size_t)total)) return ROGTK_E_HIP;
        if (int rc = rogtk_str_fill(op, dcols, n_cols, n_rows, param, c->offsets.as<int64_t>(), c->out.as<uint8_t>(),
                                    s))
            return rc;
        ROGTK_HIP_CHECK(hipMemcpyAsync(out->values, c->out.p, (size_t)total, hipMemcpyDeviceToHost, s));
        ROGTK_HIP_CHECK(hipStreamSynchronize(s));
    }
    int64_t nulls = 0;
    for (int64_t r = 0; r < n_rows; ++r) nulls += !((bits[r >> 3] >> (r & 7)) & 1);
    out->null_count = nulls;
    return ROGTK_OK;
}

void rogtk_str_result_free(rogtk_str_result* r) {
    if (!r) return;
    free(r->offsets);
    free(r->values);
    free(r->validity);
    *r = rogtk_str_result{};
}

}  // extern "C"
