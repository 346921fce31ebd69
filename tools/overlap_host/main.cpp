// The line-overlap core (plankassembly_amd/csrc/overlap_core.h) on the host, as a program of its own: what csrc/overlap.hip
// computes per pair, serially, from a text file of cases.  tests/test_reprojection_cpu.py builds it with the host compiler and
// compares it with the raster of tests/reprojection_reference.py; build it with -fsanitize=address,undefined and run it (this
// program only, never loaded into python) to check the core's bounds: every row and the work area are heap blocks of exactly
// the size the kernel is given.
//
//   c++ -std=c++17 -O1 -g [-fsanitize=address,undefined -fno-sanitize-recover=all] -o overlap_host tools/overlap_host/main.cpp
//   overlap_host cases.txt
//
// cases.txt:  n_pairs
//             then per pair a line "end_token num_bits tol mode" (mode 0 ignore, 1 match, 2 visible) and, for side a and then
//             side b, a line "len has_type" followed by the value row, the view row and - with has_type - the type row, len
//             integers each.
// Output: one line of the eight counts per pair.  What the library refuses (a row that holds more than 1024 lines, num_bits outside
// 1 .. 11, tol outside 0 .. 255, a bad mode, mode 1 without both type rows): "error" and exit status 2.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "../../plankassembly_amd/csrc/overlap_core.h"

struct Side {
    int64_t *value = nullptr, *view = nullptr, *type = nullptr;
    int len = 0;
    ~Side() { delete[] value; delete[] view; delete[] type; }
};

static bool read_row(FILE* f, int64_t** row, int len) {
    *row = new int64_t[len];                                    // exactly len: a read past the row is a heap overflow
    for (int i = 0; i < len; ++i)
        if (fscanf(f, "%" SCNd64, *row + i) != 1) return false;
    return true;
}

static bool read_side(FILE* f, Side* s) {
    int has_type;
    if (fscanf(f, "%d %d", &s->len, &has_type) != 2 || s->len < 0 || ov_lines(s->len) > OV_MAX_LINES) return false;
    if (!read_row(f, &s->value, s->len) || !read_row(f, &s->view, s->len)) return false;
    return !has_type || read_row(f, &s->type, s->len);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 1; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 1; }
    int n_pairs;
    if (fscanf(f, "%d", &n_pairs) != 1) { puts("error"); return 2; }
    for (int p = 0; p < n_pairs; ++p) {
        int end_token, num_bits, tol, mode;
        Side a, b;
        if (fscanf(f, "%d %d %d %d", &end_token, &num_bits, &tol, &mode) != 4 || num_bits < 1 || num_bits > OV_MAX_BITS || tol < 0 ||
            tol > OV_MAX_TOL || mode < OV_MODE_IGNORE || mode > OV_MODE_VISIBLE || !read_side(f, &a) || !read_side(f, &b) ||
            (mode == OV_MODE_MATCH && (!a.type || !b.type))) {
            puts("error");
            return 2;
        }
        const OvLayout l = ov_layout(a.len, b.len);
        unsigned char* mem = static_cast<unsigned char*>(aligned_alloc(16, (size_t)l.bytes));
        int32_t out[8];
        ov_pair_serial(a.value, a.view, a.type, a.len, b.value, b.view, b.type, b.len, end_token, num_bits, tol, mode, mem, out);
        printf("%d %d %d %d %d %d %d %d\n", out[0], out[1], out[2], out[3], out[4], out[5], out[6], out[7]);
        free(mem);
    }
    fclose(f);
    return 0;
}
