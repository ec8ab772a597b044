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

#include "column_util.h"
#include "level2.h"
#include "strings_rows.h"

namespace rogtk {
namespace {

using namespace str_rows;

constexpr int kBlock = 256;

// An input column as the kernels take it: a DevCol whose row count gives way to the
// broadcast flag (the rows of a call are OpArgs::n).
struct Col {
    const void* off;
    int ow;
    const uint8_t* val;
    const uint8_t* valid;
    int64_t voff;
    int bcast;  // row 0 for every row (a length-1 column broadcast)
};
Col as_col(const DevCol& d, int64_t n_rows) {
    return Col{d.offsets, d.ow, d.values, d.validity, d.voff, d.n == 1 && n_rows != 1 ? 1 : 0};
}

struct Cols {
    Col c[3];
};

__device__ __forceinline__ bool col_valid(const Col& c, int64_t i) {
    return row_valid(c.valid, c.voff, c.bcast ? 0 : i);
}

__device__ __forceinline__ Str col_str(const Col& c, int64_t i) {
    if (c.bcast) i = 0;
    const int64_t a = row_off(c.off, c.ow, i), b = row_off(c.off, c.ow, i + 1);
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
        a->cols.c[k] = as_col(DevCol(c.offsets, c.offset_width, c.values, c.validity, c.validity_offset, c.n), n_rows);
    }
    return ROGTK_OK;
}

inline unsigned grid_rows(int64_t n) { return (unsigned)std::max<int64_t>((n + kBlock - 1) / kBlock, 1); }

// the two passes over columns already checked (make_args), for the device and the host entries
int measure(const OpArgs& a, int64_t* out_offsets, uint64_t* out_valid_bits, void* temp, int64_t temp_bytes,
            hipStream_t s) {
    const int64_t n_rows = a.n;
    ROGTK_REQUIRE(n_rows < (int64_t)1 << 31, ROGTK_E_UNSUPPORTED, "at most 2^31 - 1 rows per call");
    ROGTK_REQUIRE(out_offsets && out_valid_bits && temp, ROGTK_E_INVALID, "null output / temp pointer");
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

int fill(const OpArgs& a, const int64_t* offsets, uint8_t* out_values, hipStream_t s) {
    if (a.n > 0) hipLaunchKernelGGL(k_str_fill, dim3(grid_rows(a.n)), dim3(kBlock), 0, s, a, offsets, out_values);
    ROGTK_HIP_CHECK(hipGetLastError());
    return ROGTK_OK;
}

// The host entry after its checks (a: the host columns as make_args took them): the columns
// onto the context's slots, the two passes, the result through the shared writer. Scratch:
// out[4] the output offsets, out[5] the scan's storage, out[6] the bytes, out[7] the validity.
int transform_host(HostCtx* c, OpArgs a, const rogtk_str_col* cols, int n_cols, rogtk_str_result* out) {
    const int64_t n = a.n;
    for (int k = 0; k < n_cols; ++k) {
        DevCol d;
        if (int rc = upload_col(c, k, HostCol(cols[k]), &d)) return rc;
        a.cols.c[k] = as_col(d, n);
    }
    int64_t tb = 0;
    if (int rc = rogtk_str_temp_bytes(n, &tb)) return rc;
    const int64_t words = std::max<int64_t>((n + 63) / 64, 1);
    if (c->out[4].ensure((size_t)(n + 1) * 8) || c->out[5].ensure((size_t)tb) || c->out[7].ensure((size_t)words * 8))
        return ROGTK_E_HIP;
    const int64_t* d_off = c->out[4].as<int64_t>();
    const uint64_t* d_valid = c->out[7].as<uint64_t>();
    if (int rc = measure(a, c->out[4].as<int64_t>(), c->out[7].as<uint64_t>(), c->out[5].p, tb, c->stream)) return rc;
    if (int rc = str_result_begin(c, n, d_off, d_valid, nullptr, out)) return rc;
    // a row over the cap (a CIGAR number far beyond its sequences): an error before the
    // output is allocated or filled
    for (int64_t r = 0; r < n; ++r)
        ROGTK_REQUIRE(out->offsets[r + 1] - out->offsets[r] <= ROGTK_STR_MAX_ROW_BYTES, ROGTK_E_UNSUPPORTED,
                      "row %lld: the output is longer than ROGTK_STR_MAX_ROW_BYTES (%lld bytes)", (long long)r,
                      (long long)ROGTK_STR_MAX_ROW_BYTES);
    return str_result_finish(c, c->out[6], [&](uint8_t* d) { return fill(a, d_off, d, c->stream); }, out);
}

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
    return measure(a, out_offsets, out_valid_bits, temp, temp_bytes, as_stream(stream));
}

int rogtk_str_fill(int op, const rogtk_str_col* cols, int n_cols, int64_t n_rows, int64_t param,
                   const int64_t* offsets, uint8_t* out_values, void* stream) {
    OpArgs a;
    if (int rc = make_args(op, cols, n_cols, n_rows, param, &a)) return rc;
    return fill(a, offsets, out_values, as_stream(stream));
}

int rogtk_str_transform_host(int op, const rogtk_str_col* cols, int n_cols, int64_t n_rows, int64_t param,
                             rogtk_str_result* out) {
    ROGTK_REQUIRE(out && cols, ROGTK_E_INVALID, "null argument");
    *out = rogtk_str_result{};
    OpArgs a;
    if (int rc = make_args(op, cols, n_cols, n_rows, param, &a)) return rc;
    HostCtx* c;
    if (int rc = host_ctx(&c)) return rc;
    const int rc = transform_host(c, a, cols, n_cols, out);
    if (rc) rogtk_str_result_free(out);
    return rc;
}

void rogtk_str_result_free(rogtk_str_result* r) {
    if (!r) return;
    free(r->offsets);
    free(r->values);
    free(r->validity);
    *r = rogtk_str_result{};
}

}  // extern "C"

