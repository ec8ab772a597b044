// strings_rows.h — the row functions of the element-wise string transforms
// (strings.hip), compiled for the device by hipcc and for the host by any C++17
// compiler (oracle/str_rows_host.cpp runs them under the host sanitizers).
//
// Each op is ONE function over a row, instantiated with a counting (FILL = false)
// and a writing (FILL = true) emitter. Arithmetic follows the reference's release
// build (Cargo.toml [profile.release]: no overflow checks): usize sums wrap,
// `u8 - base` wraps.
//
// Bounds. A CIGAR number, not the input length, decides how much a row emits, so:
//   * the counting emitter saturates at ROGTK_STR_MAX_ROW_BYTES + 1 ("over the cap"),
//     and a row over the cap is never filled (the callers skip it);
//   * every loop whose trip count is a CIGAR number is checked against the room left
//     under the cap before it starts, so an over-cap row costs time proportional to
//     its input bytes;
//   * an insertion is recorded only when it lies inside the sequence, tested without a
//     wrapping sum: no pointer outside a row is ever formed.
#pragma once

#include <stdint.h>

#include "../../include/rogtk_hip.h"

#if defined(__HIPCC__)
#define ROGTK_HD __host__ __device__
#define ROGTK_HD_INLINE __host__ __device__ __forceinline__
#else
#define ROGTK_HD
#define ROGTK_HD_INLINE inline
#endif

namespace rogtk {
namespace str_rows {

constexpr uint64_t kRowCap = ROGTK_STR_MAX_ROW_BYTES;

struct Str {
    const uint8_t* p;
    uint64_t n;
};

ROGTK_HD_INLINE uint64_t min_u64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// Counting (FILL = false) or writing (FILL = true) output bytes. The counting emitter
// keeps n <= kRowCap + 1; the writing one only ever runs on rows within the cap.
template <bool FILL>
struct Emit {
    uint8_t* p;
    uint64_t n = 0;
    ROGTK_HD_INLINE bool over() const { return n > kRowCap; }
    ROGTK_HD_INLINE uint64_t room() const { return kRowCap - n; }  // bytes left under the cap (n <= kRowCap)
    ROGTK_HD_INLINE void overflow() { n = kRowCap + 1; }
    ROGTK_HD_INLINE void advance(uint64_t k) {
        if (FILL)
            n += k;
        else
            n = k > kRowCap + 1 - n ? kRowCap + 1 : n + k;
    }
    ROGTK_HD_INLINE void put(uint8_t b) {
        if (FILL) p[n] = b;
        advance(1);
    }
    ROGTK_HD_INLINE void fill(uint8_t b, uint64_t k) {
        if (FILL)
            for (uint64_t j = 0; j < k; ++j) p[n + j] = b;
        advance(k);
    }
    ROGTK_HD_INLINE void bytes(const uint8_t* s, uint64_t k) {
        if (FILL)
            for (uint64_t j = 0; j < k; ++j) p[n + j] = s[j];
        advance(k);
    }
    // `format!("{}", v)` of a usize / u8
    ROGTK_HD_INLINE void dec(uint64_t v) {
        uint8_t t[20];
        int k = 0;
        do {
            t[k++] = (uint8_t)('0' + v % 10);
            v /= 10;
        } while (v);
        while (k) put(t[--k]);
    }
    // `String::push((b as char).to_ascii_{upper,lower}case())`: a byte >= 0x80 is the
    // Latin-1 char U+00XX, two bytes of UTF-8 in the output
    ROGTK_HD_INLINE void latin1(uint8_t b, bool upper) {
        if (b < 0x80) {
            if (upper && b >= 'a' && b <= 'z') b -= 32;
            if (!upper && b >= 'A' && b <= 'Z') b += 32;
            put(b);
        } else {
            put((uint8_t)(0xC0 | (b >> 6)));
            put((uint8_t)(0x80 | (b & 0x3F)));
        }
    }
    // String::from_utf8_lossy of s[a, a + k) where s is valid UTF-8: continuation bytes
    // cut off from their lead are one U+FFFD each; a sequence cut at the end is one
    ROGTK_HD void lossy(const uint8_t* s, uint64_t k) {
        uint64_t j = 0;
        while (j < k && (s[j] & 0xC0) == 0x80) {
            put(0xEF), put(0xBF), put(0xBD);
            ++j;
        }
        while (j < k) {
            const uint8_t b = s[j];
            const uint64_t w = b < 0x80 ? 1 : b < 0xE0 ? 2 : b < 0xF0 ? 3 : 4;
            if (j + w > k) {
                put(0xEF), put(0xBF), put(0xBD);
                return;
            }
            bytes(s + j, w);
            j += w;
        }
    }
};

// CIGAR tokenizer of the reference loops: digits accumulate (`is_ascii_digit`), any
// other char ends a token; `num_buf.parse::<usize>()` fails on an empty buffer or
// on overflow, and a failed parse skips the op. Multi-byte chars: their lead byte
// ends the token (an unknown op), their continuation bytes see an empty buffer.
struct CigarTok {
    const uint8_t* s;
    uint64_t n, j = 0;
    ROGTK_HD bool next(uint8_t* op, uint64_t* len) {
        uint64_t v = 0;
        bool digits = false, over = false;
        while (j < n) {
            const uint8_t c = s[j++];
            if (c >= '0' && c <= '9') {
                const uint64_t d = c - '0';
                if (v > (~0ull - d) / 10) over = true;
                v = v * 10 + d;
                digits = true;
                continue;
            }
            if (digits && !over) {
                *op = c;
                *len = v;
                return true;
            }
            v = 0;
            digits = over = false;
        }
        return false;
    }
};

// ---------------------------------------------------------------- the ops
template <bool F>
ROGTK_HD void op_revcomp(Emit<F>& o, Str s) {
    // dna.chars().rev(): whole UTF-8 chars in reverse order, ASCII A/T/C/G/N mapped
    uint64_t e = s.n;
    while (e > 0) {
        uint64_t b = e - 1;
        while (b > 0 && (s.p[b] & 0xC0) == 0x80) --b;
        if (e - b == 1) {
            uint8_t c = s.p[b];
            c = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
            o.put(c);
        } else {
            o.bytes(s.p + b, e - b);
        }
        e = b;
    }
}

template <bool F>
ROGTK_HD void op_parse_cigar(Emit<F>& o, Str cig, bool block_dels) {
    CigarTok t{cig.p, cig.n};
    uint8_t op;
    uint64_t len, ref = 0;
    bool first = true;
    auto sep = [&] {
        if (!first) o.put('|');
        first = false;
    };
    while (t.next(&op, &len)) {
        if (op == 'D') {
            if (block_dels) {
                sep();
                o.put('D'), o.put(','), o.dec(ref), o.put(','), o.dec(len);
            } else {
                const uint64_t end = ref + len;  // wrapping, as the release build
                if (ref < end) {
                    // len records of at least 5 bytes ("D,p,1"): past the room left, the
                    // row is over the cap whatever follows, and the loop is not entered
                    if (!F && (o.over() || len > o.room() / 5)) {
                        o.overflow();
                        return;
                    }
                    for (uint64_t p = ref; p < end; ++p) {
                        sep();
                        o.put('D'), o.put(','), o.dec(p), o.put(','), o.put('1');
                    }
                }
            }
            ref += len;
        } else if (op == 'I') {
            sep();
            o.put('I'), o.put(','), o.dec(ref), o.put(','), o.dec(len);
        } else {
            ref += len;
        }
    }
}

// expand_cigar_alignment: side 0 = aligned reference, 1 = aligned query. The copy
// loops are bounded by the input rows (rk, qk); fill() counts in O(1).
template <bool F>
ROGTK_HD void op_aligned(Emit<F>& o, Str ref, Str qry, Str cig, int side) {
    CigarTok t{cig.p, cig.n};
    uint8_t op;
    uint64_t len, rp = 0, qp = 0;
    while (t.next(&op, &len)) {
        const uint64_t rk = min_u64(len, ref.n - rp), qk = min_u64(len, qry.n - qp);
        switch (op) {
            case 'M':
            case '=':
            case 'X':
                if (side == 0)
                    for (uint64_t j = 0; j < rk; ++j) o.latin1(ref.p[rp + j], true);
                else
                    for (uint64_t j = 0; j < qk; ++j) o.latin1(qry.p[qp + j], true);
                rp += rk;
                qp += qk;
                break;
            case 'I':
                if (side == 0)
                    o.fill('-', len);
                else
                    for (uint64_t j = 0; j < qk; ++j) o.latin1(qry.p[qp + j], true);
                qp += qk;
                break;
            case 'D':
            case 'N':
                if (side == 0)
                    for (uint64_t j = 0; j < rk; ++j) o.latin1(ref.p[rp + j], true);
                else
                    o.fill('-', len);
                rp += rk;
                break;
            case 'S':
                if (side == 0)
                    o.fill('-', len);
                else
                    for (uint64_t j = 0; j < qk; ++j) o.latin1(qry.p[qp + j], false);
                qp += qk;
                break;
            default:  // 'H', 'P', unknown
                break;
        }
    }
}

// extract_insertions_from_cigar: calls fn(ref_pos, seq_pos, len) for every insertion
// the reference inserts into its HashMap (in walk order; later ones overwrite).
// seq_pos wraps as in the release build, but an insertion is reported only when
// [seq_pos, seq_pos + len) lies inside seq: the reference's own test is the wrapped
// `seq_pos + len <= seq.len()`, after which it panics on the slice (a wrapped row
// counts as "insertion past the end of seq" here).
template <class Fn>
ROGTK_HD void walk_insertions(Str seq, Str cig, Fn&& fn) {
    CigarTok t{cig.p, cig.n};
    uint8_t op;
    uint64_t len, sp = 0, rp = 0;
    while (t.next(&op, &len)) {
        switch (op) {
            case 'M':
            case '=':
            case 'X':
                sp += len;
                rp += len;
                break;
            case 'I':
                if (sp <= seq.n && len <= seq.n - sp) fn(rp, sp, len);
                sp += len;
                break;
            case 'D':
            case 'N':
                rp += len;
                break;
            case 'S':
                sp += len;
                break;
            default:
                break;
        }
    }
}

template <bool F>
ROGTK_HD void op_insertions(Emit<F>& o, Str seq, Str cig) {
    // map keys ascend in walk order (ref_pos never decreases), so sorting the map is
    // the walk order with each run of equal keys reduced to its last insertion
    bool have = false, first = true;
    uint64_t pr = 0, ps = 0, pl = 0;
    auto flush = [&] {
        if (!first) o.put('|');
        first = false;
        o.dec(pr);
        o.put(':');
        o.lossy(seq.p + ps, pl);
    };
    walk_insertions(seq, cig, [&](uint64_t r, uint64_t s, uint64_t l) {
        if (have && r != pr) flush();
        have = true;
        pr = r, ps = s, pl = l;
    });
    if (have) flush();
}

// `str::parse::<usize>()`: optional '+', then >= 1 ASCII digits, no overflow
ROGTK_HD inline bool parse_usize(const uint8_t* s, uint64_t n, uint64_t* v) {
    uint64_t j = 0;
    if (n > 0 && s[0] == '+') j = 1;
    if (j == n) return false;
    uint64_t x = 0;
    for (; j < n; ++j) {
        const uint8_t c = s[j];
        if (c < '0' || c > '9') return false;
        const uint64_t d = c - '0';
        if (x > (~0ull - d) / 10) return false;
        x = x * 10 + d;
    }
    *v = x;
    return true;
}

// the last insertion at ref_pos key (HashMap::get after all inserts)
ROGTK_HD inline bool find_insertion(Str seq, Str cig, uint64_t key, uint64_t* s_out, uint64_t* l_out) {
    bool hit = false;
    walk_insertions(seq, cig, [&](uint64_t r, uint64_t s, uint64_t l) {
        if (r == key) {
            hit = true;
            *s_out = s;
            *l_out = l;
        }
    });
    return hit;
}

template <bool F>
ROGTK_HD void op_enrich(Emit<F>& o, Str al, Str seq, Str cig, bool have_ins) {
    if (!have_ins) {  // seq or CIGAR null: the allele as is
        o.bytes(al.p, al.n);
        return;
    }
    uint64_t j = 0;
    while (j < al.n) {
        const uint8_t c = al.p[j];
        if (c != '[') {
            o.put(c);
            ++j;
            continue;
        }
        uint64_t k = j + 1;
        while (k < al.n && al.p[k] != ']') ++k;
        const uint8_t* ct = al.p + j + 1;
        const uint64_t cn = k - j - 1;
        o.put('[');
        o.bytes(ct, cn);
        if (k == al.n) return;  // no closing bracket: '[' + the rest
        // "pos:...I" -> the insertion at pos - 1 (or pos): append ":SEQ"
        uint64_t colon = 0;
        while (colon < cn && ct[colon] != ':') ++colon;
        // split_once(':') -> (pos_str, rest); rest.ends_with('I') needs a non-empty rest
        uint64_t pos;
        if (colon + 1 < cn && ct[cn - 1] == 'I' && parse_usize(ct, colon, &pos)) {
            uint64_t s = 0, l = 0;
            const bool hit =
                (pos > 0 && find_insertion(seq, cig, pos - 1, &s, &l)) || find_insertion(seq, cig, pos, &s, &l);
            if (hit) {
                o.put(':');
                o.lossy(seq.p + s, l);
            }
        }
        o.put(']');
        j = k + 1;
    }
}

// `phred_char as u8 - base` per char (low 8 bits of the code point, wrapping)
template <bool F>
ROGTK_HD void op_phred(Emit<F>& o, Str s, uint8_t base, bool as_text) {
    uint64_t j = 0;
    bool first = true;
    while (j < s.n) {
        const uint8_t b = s.p[j];
        uint32_t cp;
        uint64_t w;
        if (b < 0x80) cp = b, w = 1;
        else if (b < 0xE0) cp = b & 0x1F, w = 2;
        else if (b < 0xF0) cp = b & 0x0F, w = 3;
        else cp = b & 0x07, w = 4;
        for (uint64_t q = 1; q < w && j + q < s.n; ++q) cp = (cp << 6) | (s.p[j + q] & 0x3F);
        j += w;
        const uint8_t v = (uint8_t)((uint8_t)cp - base);
        if (as_text) {
            if (!first) o.put('|');
            o.dec(v);
        } else {
            o.put(v);
        }
        first = false;
    }
}

// Row i of op over the input columns `in`: false = null output row. `in` is any type
// with  bool valid(int k, int64_t i)  and  Str str(int k, int64_t i)  for column k
// (broadcast and the validity / offset layout are the accessor's business).
template <bool F, class Rows>
ROGTK_HD bool run_row(int op, int64_t param, const Rows& in, int64_t i, Emit<F>& o) {
    switch (op) {
        case ROGTK_STR_REVCOMP:
            if (!in.valid(0, i)) return false;
            op_revcomp(o, in.str(0, i));
            return true;
        case ROGTK_STR_PARSE_CIGAR:
            if (!in.valid(0, i)) return false;
            op_parse_cigar(o, in.str(0, i), param != 0);
            return true;
        case ROGTK_STR_ALIGNED_REF:
        case ROGTK_STR_ALIGNED_QUERY:
            if (!in.valid(0, i) || !in.valid(1, i) || !in.valid(2, i)) return false;
            op_aligned(o, in.str(0, i), in.str(1, i), in.str(2, i), op == ROGTK_STR_ALIGNED_REF ? 0 : 1);
            return true;
        case ROGTK_STR_CIGAR_INSERTIONS:
            if (!in.valid(0, i) || !in.valid(1, i)) return false;
            op_insertions(o, in.str(0, i), in.str(1, i));
            return true;
        case ROGTK_STR_ENRICH_ALLELE: {
            if (!in.valid(0, i)) return false;
            const bool both = in.valid(1, i) && in.valid(2, i);
            const Str none{nullptr, 0};
            op_enrich(o, in.str(0, i), both ? in.str(1, i) : none, both ? in.str(2, i) : none, both);
            return true;
        }
        case ROGTK_STR_PHRED_STR:
        case ROGTK_STR_PHRED_LIST:
            if (!in.valid(0, i)) return false;
            op_phred(o, in.str(0, i), (uint8_t)param, op == ROGTK_STR_PHRED_STR);
            return true;
        default:
            return false;
    }
}

}  // namespace str_rows
}  // namespace rogtk
