// fuzzy.hip — the reference's `fuzzy` expression namespace on gfx950: one-edit pattern
// match and replace over a string column (src/expressions.rs:983-1216).
//
// The reference builds a regex from a literal target (generate_fuzzy_pattern, :983-1013)
// and hands it to the Rust `regex` crate. The patterns it can build are a closed grammar
// (include/rogtk_hip.h): an ordered alternation of sequences of literal bytes, "any code
// point but '\n'" and "optionally one such code point". This file compiles that grammar
// into a flat program on the host and matches it on the GPU with leftmost-first semantics;
// there is no regex engine and nothing outside the grammar is accepted.
//
// Lane mapping. A wavefront owns 64 consecutive rows (one word of the result bitmaps) and
// walks them one after the other; for the row in hand its 64 lanes take 64 consecutive
// start offsets, so the first byte each lane looks at is one coalesced read of the row.
// Every lane tests the alternatives in program order at its own start (the program sits
// in LDS); a ballot and find-first-set give the leftmost matching start, the winning
// lane's end offset is broadcast, and the next 64 starts are tried only when no lane hit.
// A match may extend past the 64 starts of its chunk: a lane reads as far as its
// alternative goes, bounded by the row's end only. Rows are not split over sub-wave
// groups: a 150-byte read is three chunks, and a short row costs one.
//
// What a lane does at its start is bounded by instruction issue, not by memory (measured:
// staging the bytes in LDS alone changed little), so the work per alternative is cut down
// in three steps, none of which decides a match on its own:
//   * the chunk's bytes [c, c + 256) are staged in LDS once (four coalesced reads per
//     wave) and each lane keeps its first 8 bytes in a register;
//   * a prefilter per alternative (two masked 8-byte compares precomputed on the host:
//     the literals before the first wildcard, and those after it at the one or two
//     places they can start) rejects nearly every start of a random read;
//   * the lane measures once how far the row agrees with the program's longest literal
//     run (for a generated pattern: the target itself); alternatives that repeat that
//     run at the same positions, as all variants of one target do, skip or fail those
//     atoms from the measured length, so a near-match costs O(L) steps, not O(L^2).
// Whatever passes is verified atom by atom (run_plain / match_alt), the only code that
// knows about code-point widths, '\n' and the row's end.
// Because a wave owns a whole bitmap word it writes the result and validity words with
// one plain store each (no atomics), and the offsets of its 64 rows arrive in one
// coalesced load that is then broadcast row by row.
//
// Replace is measure-then-fill like strings.hip: the measuring pass writes the output
// byte length of every row, the lengths are scanned into offsets, and the filling pass
// FINDS THE MATCHES AGAIN and copies the pieces with all 64 lanes. Recording the matches
// instead would need a per-row list of unbounded length for replace_all; the search is
// the cheaper half of the fill (which also moves every byte of the column), and running
// the same device function twice keeps the two passes from disagreeing.
#include <hipcub/hipcub.hpp>

#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "column_util.h"
#include "level2.h"

namespace {

constexpr uint16_t kAny = 256, kOpt = 257;  // atoms 0..255 are LIT(byte)
constexpr uint32_t kNoOpt = 0xFFFF;
constexpr int64_t kMaxTarget = 100;      // the reference's default max_length
constexpr size_t kMaxAlts = 512;
constexpr size_t kMaxAtoms = 16 * 1024;  // 32 KiB of LDS (+ 24 KiB of alternatives + the windows: below 64 KiB)
constexpr int kHeadWords = 8;            // n_alt, n_atoms, repl_len, lds_words, reference run: first atom, length
constexpr int kAltWords = 12;            // per alternative: first atom, len | opt << 16, the prefilter (below)

using Alt = std::vector<uint16_t>;

}  // namespace

// Device blob (uint32 words): head[4]; per alternative {first atom, len | opt_pos << 16, the
// prefilter}; the atoms, two per word; then (not copied to LDS) the replacement bytes.
struct rogtk_fuzzy_program {
    std::vector<Alt> alts;
    bool literal = false;
    std::string repl;
    std::mutex mu;
    std::map<int, void*> dev;  // device ordinal -> uploaded blob
    uint32_t lds_bytes = 0;
};

namespace rogtk {
namespace {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;

bool is_alnum(uint8_t c) { return (c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); }

std::string show(const uint8_t* s, int64_t n) {
    std::string o;
    for (int64_t i = 0; i < n && i < 48; ++i) {
        char b[8];
        if (s[i] >= 0x20 && s[i] < 0x7F)
            o += (char)s[i];
        else
            snprintf(b, sizeof b, "\\x%02x", s[i]), o += b;
    }
    if (n > 48) o += "...";
    return o;
}

// The per-alternative limits and the de-duplication; `what` names the source in messages.
int finish_program(std::vector<Alt>&& alts, bool literal, const char* what, rogtk_fuzzy_program** out) {
    std::vector<Alt> keep;
    size_t atoms = 0;
    for (size_t a = 0; a < alts.size(); ++a) {
        const Alt& alt = alts[a];
        size_t opts = 0, must = 0;
        for (uint16_t t : alt) (t == kOpt ? opts : must) += 1;
        ROGTK_REQUIRE(must > 0, ROGTK_E_UNSUPPORTED,
                      "%s: alternative %zu can match the empty string (not supported)", what, a);
        ROGTK_REQUIRE(opts <= 1, ROGTK_E_UNSUPPORTED,
                      "%s: alternative %zu has %zu optional wildcards (at most one is supported)", what, a, opts);
        ROGTK_REQUIRE(alt.size() < kNoOpt, ROGTK_E_UNSUPPORTED, "%s: alternative %zu is too long", what, a);
        bool dup = false;
        for (const Alt& k : keep) dup = dup || k == alt;
        if (dup) continue;
        atoms += alt.size();
        keep.push_back(alt);
    }
    ROGTK_REQUIRE(!keep.empty(), ROGTK_E_UNSUPPORTED, "%s: the pattern is empty (it would match everywhere)", what);
    ROGTK_REQUIRE(keep.size() <= kMaxAlts && atoms <= kMaxAtoms, ROGTK_E_UNSUPPORTED,
                  "%s: the program has %zu alternatives and %zu atoms (at most %zu and %zu)", what, keep.size(),
                  atoms, kMaxAlts, kMaxAtoms);
    auto* p = new rogtk_fuzzy_program();
    p->alts = std::move(keep);
    p->literal = literal;
    *out = p;
    return ROGTK_OK;
}

std::vector<uint32_t> build_blob(const rogtk_fuzzy_program& p) {
    const size_t na = p.alts.size();
    size_t atoms = 0;
    for (const Alt& a : p.alts) atoms += a.size();
    const size_t lds_words = kHeadWords + kAltWords * na + (atoms + 1) / 2;
    std::vector<uint32_t> b(lds_words + (p.repl.size() + 3) / 4 + 1, 0);
    b[0] = (uint32_t)na, b[1] = (uint32_t)atoms, b[2] = (uint32_t)p.repl.size(), b[3] = (uint32_t)lds_words;
    uint16_t* at = (uint16_t*)(b.data() + kHeadWords + kAltWords * na);
    // The reference run: the longest run of leading literals of any alternative. A lane
    // measures once how far the row agrees with it at its start (m bytes); alternatives
    // that repeat the run's atoms at the same positions are then judged from m alone.
    size_t ref = 0, ref_len = 0;
    auto lit_run = [](const Alt& alt) {
        size_t k = 0;
        while (k < alt.size() && alt[k] < 256) ++k;
        return k;
    };
    for (size_t a = 0; a < na; ++a)
        if (lit_run(p.alts[a]) > ref_len) ref = a, ref_len = lit_run(p.alts[a]);
    const Alt& R = p.alts[ref];
    size_t pos = 0;
    for (size_t a = 0; a < na; ++a) {
        const Alt& alt = p.alts[a];
        uint32_t opt = kNoOpt;
        if (a == ref) b[4] = (uint32_t)pos, b[5] = (uint32_t)ref_len;
        uint32_t* e = b.data() + kHeadWords + kAltWords * a;
        for (size_t k = 0; k < alt.size(); ++k) {
            if (alt[k] == kOpt) opt = (uint32_t)k;
            at[pos + k] = alt[k];
        }
        e[0] = (uint32_t)pos;
        e[1] = (uint32_t)alt.size() | (opt << 16);
        // The prefilter, a necessary condition on the 8 bytes at the start: the literal atoms
        // before the first wildcard (one byte each), and, when that wildcard is among the
        // first 8 atoms, its kind (1 ANY, 2 OPT), position j and the literals that follow it.
        uint64_t pre_lit = 0, pre_mask = 0, aft_lit = 0, aft_mask = 0;
        size_t j = 0;
        for (; j < alt.size() && j < 8 && alt[j] < 256; ++j)
            pre_lit |= (uint64_t)alt[j] << (8 * j), pre_mask |= 0xFFull << (8 * j);
        uint32_t kind = 0;
        if (j < alt.size() && j < 8) {
            kind = alt[j] == kAny ? 1 : 2;
            for (size_t q = 0; q < 8 && j + 1 + q < alt.size() && alt[j + 1 + q] < 256; ++q)
                aft_lit |= (uint64_t)alt[j + 1 + q] << (8 * q), aft_mask |= 0xFFull << (8 * q);
        }
        e[2] = (uint32_t)j | (kind << 8);
        // sp: atoms [0, sp) are the reference run's; al_end: with an OPT at o, atoms
        // [o + 1, al_end) are the reference run's at the same positions
        size_t sp = 0, al_end = 0;
        while (sp < alt.size() && sp < ref_len && alt[sp] < 256 && alt[sp] == R[sp]) ++sp;
        if (opt != kNoOpt) {
            al_end = opt + 1;
            while (al_end < alt.size() && al_end < ref_len && alt[al_end] < 256 && alt[al_end] == R[al_end]) ++al_end;
        }
        e[3] = (uint32_t)sp | ((uint32_t)al_end << 16);
        memcpy(e + 4, &pre_lit, 8), memcpy(e + 6, &pre_mask, 8);
        memcpy(e + 8, &aft_lit, 8), memcpy(e + 10, &aft_mask, 8);
        pos += alt.size();
    }
    if (!p.repl.empty()) memcpy(b.data() + lds_words, p.repl.data(), p.repl.size());
    return b;
}

// ------------------------------------------------------------------ device
constexpr int kWin = 256;  // bytes of the row staged in LDS per wave and 64-start chunk

struct Prog {  // the program in LDS, and this wave's window
    const uint32_t* alts;
    const uint16_t* atoms;
    int n_alt;
    uint8_t* win;
    const uint16_t* ref;  // the reference run (build_blob)
    int ref_len;
};

__device__ __forceinline__ int cp_width(uint8_t b) { return b < 0x80 ? 1 : b < 0xE0 ? 2 : b < 0xF0 ? 3 : 4; }

// All threads of the block: blob head + alternatives + atoms into LDS. The windows of the
// block's waves follow the program.
__device__ __forceinline__ Prog load_program(const uint32_t* __restrict__ blob, uint32_t* lds) {
    const uint32_t words = blob[3];
    for (uint32_t i = threadIdx.x; i < words; i += kBlock) lds[i] = blob[i];
    __syncthreads();
    const int na = (int)lds[0];
    const uint16_t* atoms = (const uint16_t*)(lds + kHeadWords + kAltWords * na);
    return Prog{lds + kHeadWords, atoms, na, (uint8_t*)(lds + words) + (threadIdx.x >> 6) * kWin, atoms + lds[4],
                (int)lds[5]};
}

// LDS traffic of one wave is ordered by the hardware; this keeps the compiler from moving
// the window's reads and writes across each other.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// What a lane sees of the row: its first 8 bytes from a register, the chunk's window
// [c, c + kWin) from LDS (zero past the row's end), anything further from memory.
struct RowView {
    const uint8_t* s;
    int64_t n;
    const uint8_t* win;
    int64_t c, st;
    uint64_t head;
    __device__ __forceinline__ uint8_t at(int64_t pos) const {
        const int64_t d = pos - st;
        if (d < 8) return (uint8_t)(head >> (8 * d));
        const int64_t w = pos - c;
        return w < kWin ? win[w] : s[pos];
    }
};

struct AltView {  // an alternative's atoms in LDS
    const uint16_t* a;
    __device__ __forceinline__ uint16_t atom(int k) const { return a[k]; }
};

// The prefilter of an alternative (build_blob) on a lane's first 8 bytes: false only where
// the alternative cannot match at the lane's start. Bytes past the row's end are zero.
__device__ __forceinline__ bool may_match(const uint32_t* e, uint64_t head) {
    const uint64_t pre_lit = e[4] | (uint64_t)e[5] << 32, pre_mask = e[6] | (uint64_t)e[7] << 32;
    if ((head ^ pre_lit) & pre_mask) return false;
    const uint32_t kind = e[2] >> 8;
    if (kind == 0) return true;
    const uint64_t aft_lit = e[8] | (uint64_t)e[9] << 32, aft_mask = e[10] | (uint64_t)e[11] << 32;
    const int j = (int)(e[2] & 0xFF);  // < 8
    // the literals after the wildcard at byte p of the head (what lies beyond it is not judged)
    auto after_at = [&](int p) { return ((((head >> (8 * p)) ^ aft_lit) & aft_mask) & (~0ull >> (8 * p))) == 0; };
    const int p1 = j + cp_width((uint8_t)(head >> (8 * j)));  // the wildcard takes a code point
    bool ok = p1 >= 8 || after_at(p1);
    if (kind == 2) ok = ok || after_at(j);  // or, OPT, none
    return ok;
}

// Atoms [k0, k1) hold no OPT. The end offset of their match at pos, or -1.
__device__ __forceinline__ int64_t run_plain(const AltView& a, int k0, int k1, const RowView& r, int64_t pos) {
    for (int k = k0; k < k1; ++k) {
        if (pos >= r.n) return -1;
        const uint8_t c = r.at(pos);
        const uint16_t t = a.atom(k);
        if (t < 256) {
            if (c != t) return -1;
            ++pos;
        } else {
            if (c == '\n') return -1;
            pos += cp_width(c);
            if (pos > r.n) return -1;  // a code point cut off by the row's end (not valid UTF-8)
        }
    }
    return pos;
}

// One alternative at the lane's start: its end offset or -1. OPT takes a code point first.
// m: bytes [st, st + m) equal the reference run's first m atoms and byte st + m does not
// (or lies past the row's end, or m is the run's length); sp, al_end: build_blob.
__device__ __forceinline__ int64_t match_alt(const AltView& a, int len, uint32_t opt, const RowView& r, int m, int sp,
                                             int al_end) {
    const int64_t st = r.st;
    if (m < sp) return -1;  // atom m < sp is the run's, and the row differs from it there
    if (opt == kNoOpt) return run_plain(a, sp, len, r, st + sp);
    const int j = (int)opt;
    const int64_t pos = run_plain(a, sp, j, r, st + sp);
    if (pos < 0) return -1;
    if (pos < r.n) {
        const uint8_t c = r.at(pos);
        const int64_t p2 = pos + cp_width(c);
        if (c != '\n' && p2 <= r.n) {
            int k = j + 1;
            int64_t q = p2;
            bool dead = false;
            if (p2 - st == j + 1 && m >= j + 1 && al_end > j + 1) {
                // atoms [j + 1, al_end) sit on the reference run's own positions
                if (m >= al_end)
                    k = al_end, q = st + al_end;
                else
                    dead = true;  // atom m of them meets the byte that differs
            }
            if (!dead) {
                const int64_t e = run_plain(a, k, len, r, q);
                if (e >= 0) return e;
            }
        }
    }
    return run_plain(a, j + 1, len, r, pos);
}

// The leftmost-first match of row s[0, n) starting at or after `from` (a code-point
// boundary). Called by all 64 lanes with the same arguments; the result is the same in
// every lane.
__device__ __forceinline__ bool wave_search(const Prog& p, const uint8_t* s, int64_t n, int64_t from, int64_t* mb,
                                            int64_t* me) {
    const int lane = threadIdx.x & 63;
    for (int64_t c = from; c < n; c += 64) {
        // stage [c, c + kWin): four coalesced 64-byte reads
        wave_lds_sync();
#pragma unroll
        for (int j = 0; j < kWin; j += 64) {
            const int64_t q = c + j + lane;
            p.win[j + lane] = q < n ? s[q] : (uint8_t)0;
        }
        wave_lds_sync();
        RowView r{s, n, p.win, c, c + lane, 0};
        {  // bytes [st, st + 8) out of three aligned words
            const uint32_t* w32 = (const uint32_t*)p.win + (lane >> 2);
            const uint32_t x = w32[0], y = w32[1], z = w32[2];
            const int sh = (lane & 3) * 8;
            const uint32_t lo = (uint32_t)((x | (uint64_t)y << 32) >> sh), hi = (uint32_t)((y | (uint64_t)z << 32) >> sh);
            r.head = lo | (uint64_t)hi << 32;
        }
        int64_t end = -1;
        if (r.st < n && ((uint8_t)r.head & 0xC0) != 0x80) {
            int m = 0;
            while (m < p.ref_len && r.st + m < n && r.at(r.st + m) == p.ref[m]) ++m;
            for (int a = 0; a < p.n_alt; ++a) {
                const uint32_t* e = p.alts + kAltWords * a;
                if (!may_match(e, r.head)) continue;
                const AltView av{p.atoms + e[0]};
                const uint32_t w = e[1], x = e[3];
                end = match_alt(av, (int)(w & 0xFFFF), w >> 16, r, m, (int)(x & 0xFFFF), (int)(x >> 16));
                if (end >= 0) break;
            }
        }
        const uint64_t m = __ballot(end >= 0);
        if (m) {
            const int w = __ffsll((unsigned long long)m) - 1;
            *mb = c + w;
            *me = c + __shfl((int)(end - c), w);
            return true;
        }
    }
    return false;
}

// Word w of the result: rows [64 w, 64 w + 64), lane = row within the word.
struct RowWord {
    int64_t a, b;  // this lane's row: value offsets
    uint64_t valid;
    int rows;
};
__device__ __forceinline__ RowWord load_word(const DevCol& col, int64_t w) {
    const int lane = threadIdx.x & 63;
    const int64_t i = w * 64 + lane;
    RowWord r{0, 0, 0, (int)min((int64_t)64, col.n - w * 64)};
    bool ok = false;
    if (i < col.n) {
        ok = row_valid(col.validity, col.voff, i);
        r.a = row_off(col.offsets, col.ow, i);
        r.b = row_off(col.offsets, col.ow, i + 1);
    }
    r.valid = __ballot(ok);
    return r;
}

extern __shared__ uint32_t fz_lds[];

__global__ __launch_bounds__(kBlock) void k_fuzzy_contains(const uint32_t* __restrict__ blob, DevCol col,
                                                           uint64_t* __restrict__ out_bits,
                                                           uint64_t* __restrict__ out_valid) {
    const Prog p = load_program(blob, fz_lds);
    const int lane = threadIdx.x & 63;
    const int64_t n_words = (col.n + 63) >> 6;
    for (int64_t w = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); w < n_words;
         w += (int64_t)gridDim.x * kWavesPerBlock) {
        const RowWord rw = load_word(col, w);
        uint64_t hits = 0;
        for (int r = 0; r < rw.rows; ++r) {
            const int64_t a = __shfl(rw.a, r), b = __shfl(rw.b, r);
            if (!((rw.valid >> r) & 1)) continue;
            int64_t mb, me;
            if (wave_search(p, col.values + a, b - a, 0, &mb, &me)) hits |= 1ull << r;
        }
        if (lane == 0) {
            out_bits[w] = hits;
            out_valid[w] = rw.valid;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_fuzzy_replace_measure(const uint32_t* __restrict__ blob, DevCol col,
                                                                  int replace_all, int64_t* __restrict__ lengths,
                                                                  uint64_t* __restrict__ out_valid) {
    const Prog p = load_program(blob, fz_lds);
    const int lane = threadIdx.x & 63;
    const int64_t repl_len = fz_lds[2];
    const int64_t n_words = (col.n + 63) >> 6;
    for (int64_t w = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); w < n_words;
         w += (int64_t)gridDim.x * kWavesPerBlock) {
        const RowWord rw = load_word(col, w);
        int64_t mine = 0;
        for (int r = 0; r < rw.rows; ++r) {
            const int64_t a = __shfl(rw.a, r), b = __shfl(rw.b, r);
            if (!((rw.valid >> r) & 1)) continue;
            const uint8_t* s = col.values + a;
            const int64_t n = b - a;
            int64_t pos = 0, total = n, mb, me;
            while (wave_search(p, s, n, pos, &mb, &me)) {
                total += repl_len - (me - mb);
                pos = me;
                if (!replace_all) break;
            }
            if (lane == r) mine = total;
        }
        if (lane < rw.rows) lengths[w * 64 + lane] = mine;
        if (lane == 0) out_valid[w] = rw.valid;
    }
}

__device__ __forceinline__ void wave_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, int64_t k) {
    for (int64_t j = threadIdx.x & 63; j < k; j += 64) dst[j] = src[j];
}

__global__ __launch_bounds__(kBlock) void k_fuzzy_replace_fill(const uint32_t* __restrict__ blob, DevCol col,
                                                               int replace_all,
                                                               const int64_t* __restrict__ offsets,
                                                               uint8_t* __restrict__ out) {
    const Prog p = load_program(blob, fz_lds);
    const int64_t repl_len = fz_lds[2];
    const uint8_t* repl = (const uint8_t*)(blob + fz_lds[3]);
    const int64_t n_words = (col.n + 63) >> 6;
    for (int64_t w = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); w < n_words;
         w += (int64_t)gridDim.x * kWavesPerBlock) {
        const RowWord rw = load_word(col, w);
        const int lane = threadIdx.x & 63;
        const int64_t my_o = lane < rw.rows ? offsets[w * 64 + lane] : 0;
        for (int r = 0; r < rw.rows; ++r) {
            const int64_t a = __shfl(rw.a, r), b = __shfl(rw.b, r), o0 = __shfl(my_o, r);
            if (!((rw.valid >> r) & 1)) continue;
            const uint8_t* s = col.values + a;
            const int64_t n = b - a;
            uint8_t* o = out + o0;
            int64_t pos = 0, mb, me;
            while (wave_search(p, s, n, pos, &mb, &me)) {
                wave_copy(o, s + pos, mb - pos);
                o += mb - pos;
                wave_copy(o, repl, repl_len);
                o += repl_len;
                pos = me;
                if (!replace_all) break;
            }
            wave_copy(o, s + pos, n - pos);
        }
    }
}

// ------------------------------------------------------------------ launch
int to_col(const rogtk_str_col* c, DevCol* out) {
    ROGTK_REQUIRE(c, ROGTK_E_INVALID, "null column");
    ROGTK_REQUIRE(c->offset_width == 4 || c->offset_width == 8, ROGTK_E_INVALID, "offset_width must be 4 or 8");
    ROGTK_REQUIRE(c->n >= 0 && c->n < ((int64_t)1 << 31) - 1, ROGTK_E_UNSUPPORTED, "at most 2^31 - 2 rows per call");
    *out = DevCol(c->offsets, c->offset_width, c->values, c->validity, c->validity_offset, c->n);
    return ROGTK_OK;
}

unsigned grid_words(int64_t n_rows) {
    const int64_t words = (n_rows + 63) / 64;
    return (unsigned)std::min<int64_t>(std::max<int64_t>((words + kWavesPerBlock - 1) / kWavesPerBlock, 1), 8192);
}

// The program on the current device (uploaded at its first use there).
int device_blob(rogtk_fuzzy_program* p, hipStream_t s, const uint32_t** blob, uint32_t* lds_bytes) {
    ROGTK_REQUIRE(p, ROGTK_E_INVALID, "null program");
    int dev = 0;
    ROGTK_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> g(p->mu);
    auto it = p->dev.find(dev);
    if (it == p->dev.end()) {
        const std::vector<uint32_t> b = build_blob(*p);
        void* d = nullptr;
        ROGTK_HIP_CHECK(hipMalloc(&d, b.size() * 4));
        // b dies with this scope: the copy must have left the host before it does
        hipError_t e = hipMemcpyAsync(d, b.data(), b.size() * 4, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            hipFree(d);
            ROGTK_HIP_CHECK(e);
        }
        p->lds_bytes = b[3] * 4 + kWavesPerBlock * kWin;
        it = p->dev.emplace(dev, d).first;
    }
    *blob = (const uint32_t*)it->second;
    *lds_bytes = p->lds_bytes;
    return ROGTK_OK;
}

void drop_device_copies(rogtk_fuzzy_program* p) {
    int cur = 0;
    const bool have = hipGetDevice(&cur) == hipSuccess;
    for (auto& kv : p->dev) {
        if (have) hipSetDevice(kv.first);
        hipFree(kv.second);
    }
    if (have && !p->dev.empty()) hipSetDevice(cur);
    p->dev.clear();
}

// the three launches on a checked column (to_col), for the device and the host entries
int contains(rogtk_fuzzy_program* p, const DevCol& c, uint64_t* out_bits, uint64_t* out_valid_bits, hipStream_t s) {
    ROGTK_REQUIRE(out_bits && out_valid_bits, ROGTK_E_INVALID, "null output pointer");
    const uint32_t* blob;
    uint32_t lds;
    if (int rc = device_blob(p, s, &blob, &lds)) return rc;
    if (c.n > 0)
        hipLaunchKernelGGL(k_fuzzy_contains, dim3(grid_words(c.n)), dim3(kBlock), lds, s, blob, c, out_bits,
                           out_valid_bits);
    ROGTK_HIP_CHECK(hipGetLastError());
    return ROGTK_OK;
}

int replace_measure(rogtk_fuzzy_program* p, const DevCol& c, int replace_all, int64_t* out_offsets,
                    uint64_t* out_valid_bits, void* temp, int64_t temp_bytes, hipStream_t s) {
    ROGTK_REQUIRE(out_offsets && out_valid_bits && temp, ROGTK_E_INVALID, "null output / temp pointer");
    const uint32_t* blob;
    uint32_t lds;
    if (int rc = device_blob(p, s, &blob, &lds)) return rc;
    // temp as rogtk_str_measure: lengths (n + 1 int64), then the scan's own storage
    int64_t* lengths = (int64_t*)temp;
    const size_t head = ((size_t)(c.n + 1) * 8 + 255) / 256 * 256;
    size_t tb = 0;
    ROGTK_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, lengths, out_offsets, (int)(c.n + 1), s));
    ROGTK_REQUIRE((int64_t)(head + tb) <= temp_bytes, ROGTK_E_INVALID, "temp_bytes %lld too small (need %lld)",
                  (long long)temp_bytes, (long long)(head + tb));
    ROGTK_HIP_CHECK(hipMemsetAsync(lengths + c.n, 0, 8, s));
    if (c.n > 0)
        hipLaunchKernelGGL(k_fuzzy_replace_measure, dim3(grid_words(c.n)), dim3(kBlock), lds, s, blob, c,
                           replace_all != 0, lengths, out_valid_bits);
    ROGTK_HIP_CHECK(hipGetLastError());
    ROGTK_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum((uint8_t*)temp + head, tb, lengths, out_offsets,
                                                     (int)(c.n + 1), s));
    return ROGTK_OK;
}

int replace_fill(rogtk_fuzzy_program* p, const DevCol& c, int replace_all, const int64_t* offsets,
                 uint8_t* out_values, hipStream_t s) {
    ROGTK_REQUIRE(offsets && out_values, ROGTK_E_INVALID, "null offsets / output pointer");
    const uint32_t* blob;
    uint32_t lds;
    if (int rc = device_blob(p, s, &blob, &lds)) return rc;
    if (c.n > 0)
        hipLaunchKernelGGL(k_fuzzy_replace_fill, dim3(grid_words(c.n)), dim3(kBlock), lds, s, blob, c,
                           replace_all != 0, offsets, out_values);
    ROGTK_HIP_CHECK(hipGetLastError());
    return ROGTK_OK;
}

// What the host entries ask of their column before any device access: to_col's rules, and of
// the offsets, which are host memory here, that they do not decrease and stay inside values.
// A first offset above 0 (a slice) is accepted: upload_col rebases it.
int check_host(const rogtk_str_col* h) {
    ROGTK_REQUIRE(h && h->offsets, ROGTK_E_INVALID, "null column");
    DevCol as_given;
    if (int rc = to_col(h, &as_given)) return rc;
    const HostCol c(*h);
    for (int64_t r = 0; r < c.n; ++r)
        ROGTK_REQUIRE(c.off(r) <= c.off(r + 1), ROGTK_E_INVALID, "offsets decrease at row %lld", (long long)r);
    ROGTK_REQUIRE(c.off0() >= 0 && (c.values_len < 0 || c.off(c.n) <= c.values_len), ROGTK_E_INVALID,
                  "offsets reference bytes outside values");
    return ROGTK_OK;
}

// rogtk_fuzzy_replace_host after its checks. Scratch: out[4] the output offsets, out[5] the
// scan's storage, out[6] the bytes, out[7] the validity words.
int replace_host(HostCtx* c, rogtk_fuzzy_program* p, const rogtk_str_col* col, int replace_all, rogtk_str_result* out) {
    hipStream_t s = c->stream;
    DevCol d;
    if (int rc = upload_col(c, 0, HostCol(*col), &d)) return rc;
    const int64_t n = d.n;
    int64_t tb = 0;
    if (int rc = rogtk_str_temp_bytes(n, &tb)) return rc;
    const int64_t words = std::max<int64_t>((n + 63) / 64, 1);
    if (c->out[4].ensure((size_t)(n + 1) * 8) || c->out[5].ensure((size_t)tb) || c->out[7].ensure((size_t)words * 8))
        return ROGTK_E_HIP;
    int64_t* d_off = c->out[4].as<int64_t>();
    uint64_t* d_valid = c->out[7].as<uint64_t>();
    ROGTK_HIP_CHECK(hipMemsetAsync(d_valid, 0, (size_t)words * 8, s));
    if (int rc = replace_measure(p, d, replace_all, d_off, d_valid, c->out[5].p, tb, s)) return rc;
    if (int rc = str_result_begin(c, n, d_off, d_valid, nullptr, out)) return rc;
    return str_result_finish(
        c, c->out[6], [&](uint8_t* v) { return replace_fill(p, d, replace_all, d_off, v, s); }, out);
}

}  // namespace
}  // namespace rogtk

using namespace rogtk;

extern "C" {

int rogtk_fuzzy_compile_native(const uint8_t* target, int64_t target_len, const char* wildcard,
                               int include_original, int64_t max_length, rogtk_fuzzy_program** out) {
    ROGTK_REQUIRE(out && (target || target_len == 0) && target_len >= 0 && max_length >= 0, ROGTK_E_INVALID,
                  "bad arguments");
    *out = nullptr;
    ROGTK_REQUIRE(target_len >= 1, ROGTK_E_UNSUPPORTED,
                  "fuzzy target: an empty target is an empty pattern (it would match everywhere)");
    ROGTK_REQUIRE(target_len <= kMaxTarget, ROGTK_E_UNSUPPORTED,
                  "fuzzy target: %lld characters (at most %lld are supported)", (long long)target_len,
                  (long long)kMaxTarget);
    for (int64_t i = 0; i < target_len; ++i)
        ROGTK_REQUIRE(is_alnum(target[i]), ROGTK_E_UNSUPPORTED,
                      "fuzzy target '%s': byte %lld (0x%02x) is not an ASCII letter or digit (it would be regex "
                      "syntax or a multi-byte character)",
                      show(target, target_len).c_str(), (long long)i, target[i]);
    const std::string wc = wildcard ? wildcard : ".{0,1}";
    uint16_t watom;
    if (wc == ".{0,1}" || wc == ".?")
        watom = kOpt;
    else if (wc == ".")
        watom = kAny;
    else {
        set_error("fuzzy wildcard '%s' is not supported (one of \".{0,1}\", \".?\", \".\")",
                  show((const uint8_t*)wc.data(), (int64_t)wc.size()).c_str());
        return ROGTK_E_UNSUPPORTED;
    }
    std::vector<Alt> alts;
    const Alt orig(target, target + target_len);
    if (include_original) alts.push_back(orig);
    if (target_len <= max_length) {
        for (int64_t i = 0; i < target_len; ++i) {
            Alt v = orig;
            v[i] = watom;
            alts.push_back(std::move(v));
        }
        Alt v = orig;
        v[target_len - 1] = kAny;
        alts.push_back(std::move(v));
    }
    ROGTK_REQUIRE(!alts.empty(), ROGTK_E_UNSUPPORTED,
                  "fuzzy target: include_original = false and max_length %lld < %lld characters leave an empty "
                  "pattern (it would match everywhere)",
                  (long long)max_length, (long long)target_len);
    return finish_program(std::move(alts), false, "fuzzy target", out);
}

int rogtk_fuzzy_compile_pattern(const uint8_t* pattern, int64_t n, int literal, rogtk_fuzzy_program** out) {
    ROGTK_REQUIRE(out && (pattern || n == 0) && n >= 0, ROGTK_E_INVALID, "bad arguments");
    *out = nullptr;
    std::vector<Alt> alts;
    if (literal) {
        ROGTK_REQUIRE(n >= 1, ROGTK_E_UNSUPPORTED,
                      "fuzzy pattern: an empty literal pattern matches everywhere (not supported)");
        alts.emplace_back(pattern, pattern + n);
        return finish_program(std::move(alts), true, "fuzzy pattern", out);
    }
    alts.emplace_back();
    for (int64_t i = 0; i < n;) {
        const uint8_t c = pattern[i];
        if (c == '|') {
            alts.emplace_back();
            ++i;
        } else if (is_alnum(c)) {
            alts.back().push_back(c);
            ++i;
        } else if (c == '.') {
            if (i + 1 < n && pattern[i + 1] == '?') {
                alts.back().push_back(kOpt);
                i += 2;
            } else if (i + 5 < n && memcmp(pattern + i + 1, "{0,1}", 5) == 0) {
                alts.back().push_back(kOpt);
                i += 6;
            } else {
                alts.back().push_back(kAny);
                ++i;
            }
        } else {
            set_error("fuzzy pattern '%s': byte %lld (0x%02x%s) is outside the supported grammar (ASCII letters "
                      "and digits, '.', '.?', '.{0,1}', '|')",
                      show(pattern, n).c_str(), (long long)i, c, c >= 0x20 && c < 0x7F ? "" : ", not printable");
            return ROGTK_E_UNSUPPORTED;
        }
    }
    return finish_program(std::move(alts), false, "fuzzy pattern", out);
}

int rogtk_fuzzy_set_replacement(rogtk_fuzzy_program* p, const uint8_t* replacement, int64_t len) {
    ROGTK_REQUIRE(p && (replacement || len == 0) && len >= 0, ROGTK_E_INVALID, "bad arguments");
    ROGTK_REQUIRE(len < (int64_t)1 << 31, ROGTK_E_UNSUPPORTED, "replacement of 2 GiB or more");
    if (!p->literal)
        for (int64_t i = 0; i < len; ++i)
            ROGTK_REQUIRE(replacement[i] != '$', ROGTK_E_UNSUPPORTED,
                          "fuzzy replacement '%s': '$' at byte %lld (the regex crate would expand a capture "
                          "group reference; not supported)",
                          show(replacement, len).c_str(), (long long)i);
    std::lock_guard<std::mutex> g(p->mu);
    p->repl.assign((const char*)replacement, (size_t)len);
    drop_device_copies(p);
    return ROGTK_OK;
}

void rogtk_fuzzy_free(rogtk_fuzzy_program* p) {
    if (!p) return;
    drop_device_copies(p);
    delete p;
}

int rogtk_fuzzy_describe(const rogtk_fuzzy_program* p, char* out, int64_t cap, int64_t* out_len) {
    ROGTK_REQUIRE(p && out_len, ROGTK_E_INVALID, "bad arguments");
    std::string o;
    for (size_t a = 0; a < p->alts.size(); ++a) {
        if (a) o += '|';
        for (uint16_t t : p->alts[a]) o += t == kAny ? '.' : t == kOpt ? '?' : (char)t;
    }
    *out_len = (int64_t)o.size();
    ROGTK_REQUIRE((int64_t)o.size() <= cap && (out || o.empty()), ROGTK_E_OVERFLOW, "output larger than cap");
    if (!o.empty()) memcpy(out, o.data(), o.size());
    return ROGTK_OK;
}

int rogtk_fuzzy_contains(rogtk_fuzzy_program* p, const rogtk_str_col* col, uint64_t* out_bits,
                         uint64_t* out_valid_bits, void* stream) {
    DevCol c;
    if (int rc = to_col(col, &c)) return rc;
    return contains(p, c, out_bits, out_valid_bits, as_stream(stream));
}

int rogtk_fuzzy_replace_measure(rogtk_fuzzy_program* p, const rogtk_str_col* col, int replace_all,
                                int64_t* out_offsets, uint64_t* out_valid_bits, void* temp, int64_t temp_bytes,
                                void* stream) {
    DevCol c;
    if (int rc = to_col(col, &c)) return rc;
    return replace_measure(p, c, replace_all, out_offsets, out_valid_bits, temp, temp_bytes, as_stream(stream));
}

int rogtk_fuzzy_replace_fill(rogtk_fuzzy_program* p, const rogtk_str_col* col, int replace_all,
                             const int64_t* offsets, uint8_t* out_values, void* stream) {
    DevCol c;
    if (int rc = to_col(col, &c)) return rc;
    return replace_fill(p, c, replace_all, offsets, out_values, as_stream(stream));
}

int rogtk_fuzzy_contains_host(rogtk_fuzzy_program* p, const rogtk_str_col* col, uint64_t* out_bits,
                              uint64_t* out_valid_bits) {
    ROGTK_REQUIRE(p && col && out_bits, ROGTK_E_INVALID, "null argument");
    if (int rc = check_host(col)) return rc;
    HostCtx* c;
    if (int rc = host_ctx(&c)) return rc;
    DevCol d;
    if (int rc = upload_col(c, 0, HostCol(*col), &d)) return rc;
    const int64_t words = (d.n + 63) / 64;
    if (words == 0) return ROGTK_OK;
    if (c->out[0].ensure((size_t)words * 8) || c->out[7].ensure((size_t)words * 8)) return ROGTK_E_HIP;
    if (int rc = contains(p, d, c->out[0].as<uint64_t>(), c->out[7].as<uint64_t>(), c->stream)) return rc;
    if (int rc = c->d2h(out_bits, c->out[0].p, (size_t)words * 8)) return rc;
    return out_valid_bits ? c->d2h(out_valid_bits, c->out[7].p, (size_t)words * 8) : ROGTK_OK;
}

int rogtk_fuzzy_replace_host(rogtk_fuzzy_program* p, const rogtk_str_col* col, int replace_all,
                             rogtk_str_result* out) {
    ROGTK_REQUIRE(p && col && out, ROGTK_E_INVALID, "null argument");
    *out = rogtk_str_result{};
    if (int rc = check_host(col)) return rc;
    HostCtx* c;
    if (int rc = host_ctx(&c)) return rc;
    const int rc = replace_host(c, p, col, replace_all, out);
    if (rc) rogtk_str_result_free(out);
    return rc;
}

}  // extern "C"
