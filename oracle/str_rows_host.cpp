// TEST INFRASTRUCTURE ONLY: runs the row functions of the string transforms
// (rogtk_amd/csrc/strings_rows.h, the code the GPU kernels run) on the host, so that
// rows which must never reach a GPU unchecked (CIGAR numbers near 2^64, rows over
// ROGTK_STR_MAX_ROW_BYTES) are exercised here first, plain and under
// AddressSanitizer / UBSan (`make sanitize`).
//
//   str_rows_host IN OUT
//
// IN (little-endian int64 unless noted):
//   "RSTRIN01" | op | param | n_rows | n_cols |
//   per column: n | values_len | has_validity | offsets[n + 1] | values bytes |
//               validity bytes[n] (one byte per row; only if has_validity)
//   A column of n == 1 beside n_rows > 1 is broadcast, as in the library.
// OUT:
//   "RSTROUT1" | n_rows | lengths[n_rows] | valid bytes[n_rows] | values bytes
//   lengths[i] is the measured length (0 for a null row, ROGTK_STR_MAX_ROW_BYTES + 1
//   for a row over the cap); values are the filled rows within the cap, concatenated.
//
// The same two passes as the kernels: measure, then fill into a buffer of exactly the
// measured size. Every input row and every output row lives in a heap block of its
// own exact size, so a read or write one byte outside a row is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../rogtk_amd/csrc/strings_rows.h"

using namespace rogtk::str_rows;

namespace {

struct HostCol {
    int64_t n = 0;
    std::vector<uint8_t*> row;  // one exact-size block per row
    std::vector<uint64_t> len;
    std::vector<uint8_t> valid;
};

struct HostRows {
    const HostCol* c;
    int64_t n_rows;
    int64_t at(int k, int64_t i) const { return c[k].n == 1 && n_rows != 1 ? 0 : i; }
    bool valid(int k, int64_t i) const { return c[k].valid[at(k, i)] != 0; }
    Str str(int k, int64_t i) const { return Str{c[k].row[at(k, i)], c[k].len[at(k, i)]}; }
};

[[noreturn]] void die(const char* what) {
    fprintf(stderr, "str_rows_host: %s\n", what);
    exit(2);
}

struct Reader {
    FILE* f;
    void raw(void* p, size_t n) {
        if (n && fread(p, 1, n, f) != n) die("truncated input");
    }
    int64_t i64() {
        int64_t v;
        raw(&v, 8);
        return v;
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) die("usage: str_rows_host IN OUT");
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) die("cannot open the input file");
    Reader rd{fi};
    char magic[8];
    rd.raw(magic, 8);
    if (memcmp(magic, "RSTRIN01", 8) != 0) die("bad magic");
    const int op = (int)rd.i64();
    const int64_t param = rd.i64(), n_rows = rd.i64(), n_cols = rd.i64();
    if (n_rows < 0 || n_cols < 1 || n_cols > 3) die("bad header");
    HostCol cols[3];
    for (int k = 0; k < n_cols; ++k) {
        HostCol& c = cols[k];
        c.n = rd.i64();
        const int64_t vlen = rd.i64(), has_valid = rd.i64();
        if (!(c.n == n_rows || c.n == 1) || vlen < 0) die("bad column header");
        std::vector<int64_t> off(c.n + 1);
        rd.raw(off.data(), (size_t)(c.n + 1) * 8);
        std::vector<uint8_t> val((size_t)vlen);
        rd.raw(val.data(), (size_t)vlen);
        c.valid.assign((size_t)c.n, 1);
        if (has_valid) rd.raw(c.valid.data(), (size_t)c.n);
        for (int64_t i = 0; i < c.n; ++i) {
            if (off[i] < 0 || off[i + 1] < off[i] || off[i + 1] > vlen) die("offsets outside values");
            const size_t l = (size_t)(off[i + 1] - off[i]);
            uint8_t* p = (uint8_t*)malloc(l);
            if (l) memcpy(p, val.data() + off[i], l);
            c.row.push_back(p);
            c.len.push_back(l);
        }
    }
    fclose(fi);

    const HostRows in{cols, n_rows};
    std::vector<int64_t> lengths((size_t)n_rows);
    std::vector<uint8_t> valid((size_t)n_rows);
    std::string values;
    for (int64_t i = 0; i < n_rows; ++i) {
        Emit<false> m{nullptr};
        const bool ok = run_row(op, param, in, i, m);
        valid[i] = ok;
        lengths[i] = ok ? (int64_t)m.n : 0;
        if (!ok || m.n > kRowCap) continue;  // null, or over the cap: not filled
        uint8_t* buf = (uint8_t*)malloc((size_t)m.n);
        Emit<true> w{buf};
        run_row(op, param, in, i, w);
        if (w.n != m.n) die("the fill pass wrote another length than the measure pass counted");
        values.append((const char*)buf, (size_t)w.n);
        free(buf);
    }
    for (int k = 0; k < n_cols; ++k)
        for (uint8_t* p : cols[k].row) free(p);

    FILE* fo = fopen(argv[2], "wb");
    if (!fo) die("cannot open the output file");
    fwrite("RSTROUT1", 1, 8, fo);
    fwrite(&n_rows, 8, 1, fo);
    fwrite(lengths.data(), 8, (size_t)n_rows, fo);
    fwrite(valid.data(), 1, (size_t)n_rows, fo);
    fwrite(values.data(), 1, values.size(), fo);
    if (fclose(fo) != 0) die("write failed");
    return 0;
}
