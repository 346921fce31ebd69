// The assembly-volume core (plankassembly_amd/csrc/volume_core.h) on the host, as a program of its own: what csrc/volume.hip
// computes per pair, serially, from a text file of cases.  tests/test_volume_cpu.py builds it with the host compiler under
// -fsanitize=address,undefined, runs it (this program only, never loaded into python) and compares it with the restatement of
// tests/volume_reference.py: every row, the work area and the unordered box list are heap blocks of exactly the size the kernel
// is given.
//
//   c++ -std=c++17 -O1 -g [-fsanitize=address,undefined -fno-sanitize-recover=all] -o volume_host tools/volume_host/main.cpp
//   volume_host cases.txt
//
// cases.txt:  n_pairs end_token dof
//             then per pair two lines "len t0 t1 ... t(len-1)": the row of side a, the row of side b; a len of -1 on side b's line
//             (and nothing after it) is the call without a b side (seq_b == NULL).
// Output: one line "union_a sum_a union_b sum_b inter union_ab n_a n_b" per pair.  A dof other than 6, a len above 1026, a
// negative len (but -1 on side b) or a negative n_pairs: "error" and exit status 2, as the library refuses them.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "../../plankassembly_amd/csrc/volume_core.h"

struct Row {
    int64_t* tok = nullptr;
    int len = 0;
    ~Row() { delete[] tok; }
};

static bool read_row(FILE* f, Row* row, bool may_be_absent) {
    if (fscanf(f, "%d", &row->len) != 1) return false;
    if (may_be_absent && row->len == -1) return true;
    if (row->len < 0 || row->len > PM_MAX_LEN) return false;
    row->tok = new int64_t[row->len];                           // exactly len: a read past the row is a heap overflow
    for (int i = 0; i < row->len; ++i)
        if (fscanf(f, "%" SCNd64, row->tok + i) != 1) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 1; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 1; }
    int n_pairs, end_token, dof;
    if (fscanf(f, "%d %d %d", &n_pairs, &end_token, &dof) != 3 || n_pairs < 0 || dof != PM_DOF) { puts("error"); return 2; }
    for (int p = 0; p < n_pairs; ++p) {
        Row a, b;
        if (!read_row(f, &a, false) || !read_row(f, &b, true)) { puts("error"); return 2; }
        const bool has_b = b.len >= 0;
        if (!has_b) b.len = 0;
        const PvLayout l = pv_layout(a.len, b.len);
        unsigned char* mem = static_cast<unsigned char*>(aligned_alloc(16, (size_t)l.bytes));
        int16_t* ubox = new int16_t[(size_t)PV_BOX * l.cap];
        int64_t out[PV_OUT];
        pv_pair_serial(a.tok, a.len, has_b ? b.tok : nullptr, b.len, end_token, mem, ubox, out);
        printf("%" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", out[0], out[1],
               out[2], out[3], out[4], out[5], out[6], out[7]);
        free(mem);
        delete[] ubox;
    }
    fclose(f);
    return 0;
}
