// level2.h — what the level-2 entry points (host Arrow buffers in, host buffers out) share across
// translation units (not installed): the per-thread device context, a host
// column and its upload, a device column as one value, the checks common to the entries and
// the writer of a rogtk_str_result. The definitions are in level2.hip. An entry checks its
// arguments before it asks for the context: host_ctx() is the first device access of a call.
#pragma once

#include <functional>

#include "rogtk_internal.h"

namespace rogtk {

// Host <-> device transfers of the level-2 entry points. Pinned host memory
// (hipHostMalloc / rogtk_host_alloc / hipHostRegister) moves by direct DMA. Pageable
// memory moves through two pinned staging buffers of the context, chunk by chunk, so
// the DMA of one chunk overlaps the host copy of the other; the host copies of a chunk
// are split over a few threads (a single thread's memcpy, and the first-touch page
// faults of a fresh destination, cap a pageable copy well below the PCIe link). A small
// upload (kSmallCopy) of either kind is packed into the first staging buffer behind the ones
// before it and only enqueued: no pointer query and no wait per buffer of a short column.
struct ColBufs {
    DevBuf offsets, values, validity;
};
struct HostCtx {
    int device = -1;
    hipStream_t stream = nullptr;
    ColBufs in[3];  // the input columns of a call (upload_col); slot 0 where there is one
    DevBuf codes, regbits, irr, nirr, target, out[8], ws, bitmap;
    DevBuf grp[2];  // the grouped entries: the rows' keys, the clusters' keys
    int64_t ws_L = -1, ws_maxd = -1;
    void* pin[2] = {nullptr, nullptr};  // staging for pageable host memory
    size_t pin_used = 0;  // bytes of pin[0] that small uploads still in flight may read
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

// A string column on the device, as the engines and the kernels take it (row_off and row_valid,
// column_util.h, read it).
struct DevCol {
    const void* offsets;
    int ow;
    const uint8_t* values;
    const uint8_t* validity;  // NULL: every row is valid
    int64_t voff;
    int64_t n;
    DevCol() = default;
    DevCol(const void* offsets_, int ow_, const uint8_t* values_, const uint8_t* validity_, int64_t voff_, int64_t n_)
        : offsets(offsets_), ow(ow_), values(values_), validity(validity_), voff(voff_), n(n_) {}
    // a caller's device column: 64-bit offsets, validity from bit 0
    DevCol(const int64_t* offsets_, const uint8_t* values_, const uint8_t* validity_, int64_t n_)
        : offsets(offsets_), ow(8), values(values_), validity(validity_), voff(0), n(n_) {}
};

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

int check_offset_width(int ow);
int check_host_col(const HostCol& h);
// the size limits shared by the entries that take rows and cluster ids (an entry without a
// cluster count passes 0)
int check_rows_and_clusters(const char* name, int64_t n, int64_t n_clusters);

// The offsets, values and validity of a host column onto c->in[slot], and the device column
// they make. A column whose first offset is 0 goes up as it is, in its own offset width. One
// that starts further in (a slice; the entries that take one say so, check_host_col refuses
// it) is rebased on the host: 64-bit offsets from 0 and only the bytes [off(0), off(n)).
int upload_col(HostCtx* c, int slot, const HostCol& h, DevCol* out);
// the packed codes, regular bits and irregular row list of a column (the packed engines' input:
// method="cluster", the scores, Hamming) into c->codes / regbits / irr, and c->nirr zeroed
// ([0] the irregular rows, [1] free for launch_max_len). n_irr (nullable): read back, one sync.
int stage_uploaded(HostCtx* c, const DevCol& col, int L, int64_t* n_irr, hipStream_t s);

// the longest row (of any validity) of a device column of n >= 1 rows, reduced into the zeroed
// device word `slot`; column_max_len zeroes the word first and reads it back (one sync of s);
// device_max_len does that for an uploaded column on the context's stream
int launch_max_len(const void* offsets, int ow, int64_t n, unsigned long long* slot, hipStream_t s);
int column_max_len(const void* offsets, int ow, int64_t n, unsigned long long* slot, hipStream_t s, int64_t* out);
int device_max_len(HostCtx* c, const DevCol& col, int64_t* out);

// an all-null column of n rows without bytes (n + 1 zero offsets), to be filled by the caller
int empty_str_result(int64_t n, rogtk_str_result* out);

// The one way from device offsets and a fill to a rogtk_str_result, in two steps; either frees
// and zeroes *out when it fails, and so does the entry for what fails around them.
// begin: the n + 1 offsets, the validity bytes and the null count. The offsets come from the
// device (d_offsets) with the validity words d_valid (NULL: every row valid; the caller may
// then clear rows with str_result_set_null), or, with h given, offsets and nulls are the host
// column's own (the corrected UMI column).
int str_result_begin(HostCtx* c, int64_t n, const int64_t* d_offsets, const uint64_t* d_valid, const HostCol* h,
                     rogtk_str_result* out);
inline void str_result_set_null(rogtk_str_result* r, int64_t i) {
    r->validity[i >> 3] &= (uint8_t)~(1u << (i & 7));
    ++r->null_count;
}
// finish: the values (offsets[n] bytes) allocated, filled on the device by `fill` (into `dev`,
// enqueued on the context's stream) and downloaded; no bytes, no fill
int str_result_finish(HostCtx* c, DevBuf& dev, const std::function<int(uint8_t*)>& fill, rogtk_str_result* out);
inline void u32_result_reset(rogtk_u32_result* r) {
    if (r) *r = rogtk_u32_result{0, nullptr};
}

}  // namespace rogtk
