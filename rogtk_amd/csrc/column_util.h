// column_util.h — what the engines beside the packed bitmap path share when they walk a
// device string column (long_cluster, dist_cluster, irregular, correct, directional,
// sorted_codes): row spans, the ACGT decoder, launch sizing and stream-ordered scratch.
#pragma once

#include <cassert>

#include "rogtk_internal.h"

namespace rogtk {

inline size_t al(size_t b) { return (std::max<size_t>(b, 1) + 255) / 256 * 256; }

// a byte range carved into pieces of al() bytes: take() gives a piece's offset, total the sum so far
struct Carve {
    size_t total = 0;
    size_t take(size_t bytes) {
        const size_t at = total;
        total += al(bytes);
        return at;
    }
};

// workgroups of `block` threads over n items, at most cap (grid-stride kernels pass one)
inline unsigned grid_for(int64_t n, int block, int64_t cap = 0x7FFFFFFF) {
    return (unsigned)std::min<int64_t>(cap, std::max<int64_t>(1, (n + block - 1) / block));
}

// row -> its first byte in the values buffer and its byte length (OW = offset width, 4 or 8)
template <int OW>
__device__ __forceinline__ void span(const void* offs, int64_t row, int64_t& st, int64_t& len) {
    if (OW == 4) {
        const int32_t* o = (const int32_t*)offs;
        st = o[row];
        len = (int64_t)o[row + 1] - o[row];
    } else {
        const int64_t* o = (const int64_t*)offs;
        st = o[row];
        len = o[row + 1] - o[row];
    }
}

// A/C/G/T -> 0..3, anything else (N, lower case, ...) -> -1
__device__ __forceinline__ int base_code(uint8_t ch) {
    return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : -1;
}

// Arrow validity bit of row i (validity NULL: every row is valid)
__device__ __forceinline__ bool row_valid(const uint8_t* validity, int64_t voff, int64_t i) {
    if (!validity) return true;
    const int64_t b = voff + i;
    return (validity[b >> 3] >> (b & 7)) & 1;
}

// offset i of a column whose offset width is only known at run time (ow 4 or 8)
__device__ __forceinline__ int64_t row_off(const void* offsets, int ow, int64_t i) {
    return ow == 4 ? (int64_t)((const int32_t*)offsets)[i] : ((const int64_t*)offsets)[i];
}

// One stream-ordered allocation handed out in 256-byte aligned pieces; released behind the
// work already enqueued on the stream. The caller sizes get() as the sum of al() of its takes;
// a take past that sum stops the program.
struct Arena {
    uint8_t* base = nullptr;
    size_t off = 0, cap = 0;
    hipStream_t s = nullptr;
    ~Arena() {
        if (base) (void)hipFreeAsync(base, s);
    }
    int get(size_t bytes, hipStream_t st) {
        s = st;
        cap = std::max<size_t>(bytes, 256);
        ROGTK_HIP_CHECK(hipMallocAsync((void**)&base, cap, st));
        return ROGTK_OK;
    }
    template <class T>
    T* take(int64_t count) {
        uint8_t* p = base + off;
        off += al((size_t)std::max<int64_t>(count, 1) * sizeof(T));
        assert(off <= cap);
        return (T*)p;
    }
};

// What sorted_distinct_codes (sorted_codes.hip) leaves: the counts on the host, the arrays on
// the device, alive as long as this object.
struct SortedCodes {
    int64_t n_reg = 0;        // regular rows: valid, byte length L, only ACGT
    int64_t n_irr = 0;        // the other valid rows
    int64_t max_irr_len = 0;  // byte length of the longest irregular row
    int64_t m = 0;            // distinct codes of the regular rows
    int key_bits = 0;         // bits the sort ran over (grouped: 2 L + bit_width(max_group))
    uint32_t max_group = 0, max_irr_group = 0;  // grouped: largest key of the regular / irregular rows
    const int64_t* irr = nullptr;   // [n_irr] the irregular rows, in any order
    const uint32_t* row = nullptr;  // [n_reg] the regular rows, ascending in their code
    const uint32_t* idx = nullptr;  // [n_reg] index into D of row[k]'s code
    const uint64_t* D = nullptr;    // [m] the distinct codes, ascending
    const uint32_t* C = nullptr;    // [m] rows per distinct code (only when asked for)
    int64_t* spare = nullptr;       // [4] device words for the caller (zeroed)
    Arena rows_mem, codes_mem;      // codes_mem: D, C, then the caller's extra bytes (n_reg > 0)
};

}  // namespace rogtk
