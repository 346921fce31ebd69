// The plank-matching core (plankassembly_amd/csrc/match_core.h) on the host, as a program of its own: what csrc/match.hip
// computes per pair, serially, from a text file of cases.  tests/test_match_cpu.py builds it with the host compiler and compares
// it with the restatement; build it with -fsanitize=address,undefined and run it (this program only, never loaded into python)
// to check the core's bounds: every row and the work area are heap blocks of exactly the size the kernel is given.
//
//   c++ -std=c++17 -O1 -g [-fsanitize=address,undefined -fno-sanitize-recover=all] -o match_host tools/match_host/main.cpp
//   match_host cases.txt
//
// cases.txt:  n_pairs end_token filter_a filter_b threshold      (threshold: anything strtod reads, C99 hex floats included)
//             then per pair two lines "len t0 t1 ... t(len-1)": the row of side a, the row of side b.
// Output: one line "tp n_a n_b ties" per pair.  A len outside [0, 1026] or a threshold of 0: "error" and exit status 2, as the
// library refuses them.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../plankassembly_amd/csrc/match_core.h"

static bool read_row(FILE* f, int64_t** row, int* len) {
    if (fscanf(f, "%d", len) != 1 || *len < 0 || *len > PM_MAX_LEN) return false;
    *row = new int64_t[*len];                                   // exactly len: a read past the row is a heap overflow
    for (int i = 0; i < *len; ++i)
        if (fscanf(f, "%" SCNd64, *row + i) != 1) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 1; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 1; }
    int n_pairs, end_token, filter_a, filter_b;
    char thr[128];
    if (fscanf(f, "%d %d %d %d %127s", &n_pairs, &end_token, &filter_a, &filter_b, thr) != 5) { puts("error"); return 2; }
    const double threshold = strtod(thr, nullptr);
    if (!(threshold == threshold) || threshold == 0.0) { puts("error"); return 2; }
    for (int p = 0; p < n_pairs; ++p) {
        int64_t *a = nullptr, *b = nullptr;
        int len_a = 0, len_b = 0;
        if (!read_row(f, &a, &len_a) || !read_row(f, &b, &len_b)) { puts("error"); return 2; }
        const PmLayout l = pm_layout(len_a, len_b);
        unsigned char* mem = static_cast<unsigned char*>(aligned_alloc(16, (size_t)l.bytes));
        int32_t out[4];
        pm_pair_serial(a, len_a, b, len_b, end_token, filter_a, filter_b, threshold, mem, out);
        printf("%d %d %d %d\n", out[0], out[1], out[2], out[3]);
        free(mem);
        delete[] a;
        delete[] b;
    }
    fclose(f);
    return 0;
}
