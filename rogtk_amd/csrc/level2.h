// level2.h — what the level-2 entry points (host Arrow buffers in, host buffers out) share across
// translation units (not installed): the per-thread device context, a host
// column and its upload, a device column as one value, and the checks common to the entries.
// The definitions are in capi.hip. An entry checks its arguments before it asks for the
// context: host_ctx() is the first device access of a call.
#pragma once

#include "rogtk_internal.h"

namespace rogtk {

// Host <-> device transfers of the level-2 entry points. Pinned host memory
// (hipHostMalloc / rogtk_host_alloc / hipHostRegister) moves by direct DMA. Pageable
// memory moves through two pinned staging buffers of the context, chunk by chunk, so
// the DMA of one chunk overlaps the host copy of the other; the host copies of a chunk
// are split over a few threads (a single thread's memcpy, and the first-touch page
// faults of a fresh destination, cap a pageable copy well below the PCIe link).
struct HostCtx {
    int device = -1;
    hipStream_t stream = nullptr;
    DevBuf offsets, values, validity, codes, regbits, irr, nirr, target, out[8], ws, bitmap;
    DevBuf grp[2];  // the grouped entries: the rows' keys, the clusters' keys
    int64_t ws_L = -1, ws_maxd = -1;
    void* pin[2] = {nullptr, nullptr};  // staging for pageable host memory
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~HostCtx();
    int staging();
    int d2h(void* dst, const void* src, size_t bytes);  // device -> host; complete on return
    // host -> device; enqueued on the stream (the host buffer may be reused on return)
    int h2d(void* dst, const void* src, size_t bytes);
};

// the calling thread's context on the current device; ROGTK_E_NODEVICE without one
int host_ctx(HostCtx** out);

struct HostCol {
    const void* offsets;
    int ow;
    const uint8_t* values;
    int64_t values_len;
    const uint8_t* validity;
    int64_t voff;
    int64_t n;
    explicit HostCol(const rogtk_str_col& c)
        : offsets(c.offsets), ow(c.offset_width), values(c.values), values_len(c.values_len), validity(c.validity),
          voff(c.validity_offset), n(c.n) {}
    HostCol(const void* offsets_, int ow_, const uint8_t* values_, int64_t values_len_, const uint8_t* validity_,
            int64_t voff_, int64_t n_)
        : offsets(offsets_), ow(ow_), values(values_), values_len(values_len_), validity(validity_), voff(voff_),
          n(n_) {}
    int64_t off0() const { return off(0); }
    int64_t off(int64_t i) const { return ow == 4 ? ((const int32_t*)offsets)[i] : ((const int64_t*)offsets)[i]; }
    bool valid(int64_t i) const {
        if (!validity) return true;
        const int64_t b = voff + i;
        return (validity[b >> 3] >> (b & 7)) & 1;
    }
    int first_len() const {
        for (int64_t i = 0; i < n; ++i)
            if (valid(i)) return (int)std::min<int64_t>(off(i + 1) - off(i), 1 << 30);
        return 0;
    }
};

// A string column on the device, as the engines take it.
struct DevCol {
    const void* offsets;
    int ow;
    const uint8_t* values;
    const uint8_t* validity;  // NULL: every row is valid
    int64_t voff;
    int64_t n;
    // the host column h as upload_col left it on the context's buffers
    DevCol(const HostCtx* c, const HostCol& h)
        : offsets(c->offsets.p), ow(h.ow), values(c->values.as<uint8_t>()),
          validity(h.validity ? c->validity.as<uint8_t>() : nullptr), voff(h.voff), n(h.n) {}
    // a caller's device column: 64-bit offsets, validity from bit 0
    DevCol(const int64_t* offsets_, const uint8_t* values_, const uint8_t* validity_, int64_t n_)
        : offsets(offsets_), ow(8), values(values_), validity(validity_), voff(0), n(n_) {}
};

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

int check_host_col(const HostCol& h);
// the size limits shared by the entries that take rows and cluster ids (an entry without a
// cluster count passes 0)
int check_rows_and_clusters(const char* name, int64_t n, int64_t n_clusters);

// the offsets, values and validity of a host column on the context's buffers
int upload_col(HostCtx* c, const HostCol& h);
// the packed codes, regular bits and irregular row list of a column (the packed engines' input:
// method="cluster", the scores, Hamming) into c->codes / regbits / irr, and c->nirr zeroed
// ([0] the irregular rows, [1] free for launch_max_len). n_irr (nullable): read back, one sync.
int stage_uploaded(HostCtx* c, const DevCol& col, int L, int64_t* n_irr, hipStream_t s);

// the longest row (of any validity) of a device column of n >= 1 rows, reduced into the zeroed
// device word `slot`; column_max_len zeroes the word first and reads it back (one sync of s);
// device_max_len does that for the column already uploaded to c->offsets
int launch_max_len(const void* offsets, int ow, int64_t n, unsigned long long* slot, hipStream_t s);
int column_max_len(const void* offsets, int ow, int64_t n, unsigned long long* slot, hipStream_t s, int64_t* out);
int device_max_len(HostCtx* c, int ow, int64_t n, int64_t* out);

// an all-null column of n rows without bytes (n + 1 zero offsets), to be filled by the caller
int empty_str_result(int64_t n, rogtk_str_result* out);
inline void u32_result_reset(rogtk_u32_result* r) {
    if (r) *r = rogtk_u32_result{0, nullptr};
}

}  // namespace rogtk
