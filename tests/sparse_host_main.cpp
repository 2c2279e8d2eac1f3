// Stand-alone driver of csrc/qoc_sparse_host.h (the COO -> ELLPACK builder of the sparse state-transfer path), compiled and run by tests/test_sparse.py under the
// address and undefined-behaviour sanitizers.  Usage: sparse_host_main <file>; the file holds "n count" and then count lines "row col re im" (re / im may be
// nan or inf).  Prints "ok W stored", the W * n columns and the W * n values -- or "error <cause>".  With "overflow <n>" in place of a file name it
// builds the one operator whose n * W passes int32 (a row with n entries) and prints the builder's verdict.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qoc_sparse_host.h"

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "overflow")) {
        const int n = atoi(argv[2]);
        std::vector<int32_t> row((size_t)n, 0), col((size_t)n);
        std::vector<double> val(2 * (size_t)n, 1.0);
        for (int i = 0; i < n; ++i) col[(size_t)i] = i;
        QocEllOp op;
        std::string why;
        if (qoc_ell_build(n, n, row.data(), col.data(), val.data(), op, why)) printf("ok %d %lld\n", op.W, op.stored);
        else printf("error %s\n", why.c_str());
        return 0;
    }
    if (argc != 2) { fprintf(stderr, "usage: sparse_host_main <file> | overflow <n>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int n = 0;
    long long count = 0;
    if (fscanf(f, "%d %lld", &n, &count) != 2 || count < 0) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<int32_t> row((size_t)count), col((size_t)count);
    std::vector<double> val(2 * (size_t)count);
    for (long long i = 0; i < count; ++i) {
        int r, c;
        char re[64], im[64];
        if (fscanf(f, "%d %d %63s %63s", &r, &c, re, im) != 4) { fprintf(stderr, "bad entry %lld\n", i); return 2; }
        row[(size_t)i] = r; col[(size_t)i] = c;
        val[2 * (size_t)i] = strtod(re, nullptr); val[2 * (size_t)i + 1] = strtod(im, nullptr);
    }
    fclose(f);
    QocEllOp op;
    std::string why;
    if (!qoc_ell_build(n, count, row.data(), col.data(), val.data(), op, why)) { printf("error %s\n", why.c_str()); return 0; }
    printf("ok %d %lld\n", op.W, op.stored);
    for (size_t i = 0; i < op.col.size(); ++i) printf("%d\n", (int)op.col[i]);
    for (size_t i = 0; i < op.col.size(); ++i) printf("%.17g %.17g\n", op.val[2 * i], op.val[2 * i + 1]);
    return 0;
}
