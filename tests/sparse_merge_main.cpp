// Stand-alone driver of the merged-row builder (csrc/qoc_sparse_host.h: qoc_ell_build + qoc_ell_merge), for tests/test_sparse_ensemble.py: compiled
// with -fsanitize=address,undefined so that every index the builders form is checked.
//   sparse_merge_main FILE         FILE: "n K", then per operator "count" and count lines "row col re im"
//       prints "ok Wm", then n lines len[r], then Wm * n lines "col op re im" (slot-major) -- or "error: <cause>"
//   sparse_merge_main roundtrip    the packed index at its largest column and operator: prints "col op" as unpacked
//   sparse_merge_main bign         n = 2^24 with one empty operator: prints the refusal
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "qoc_sparse_host.h"

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: sparse_merge_main FILE | roundtrip | bign\n"); return 2; }
    std::string why;
    if (!strcmp(argv[1], "roundtrip")) {
        const int col = (1 << QOC_MERGE_COL_BITS) - 1, op = QOC_MERGE_MAX_OPS - 1;
        const int32_t pk = qoc_merge_pack(col, op);
        printf("%d %d\n%d %d\n", qoc_merge_col(pk), qoc_merge_op(pk), qoc_merge_col(qoc_merge_pack(0, op)), qoc_merge_op(qoc_merge_pack(col, 0)));
        return 0;
    }
    if (!strcmp(argv[1], "bign")) {
        const int n = 1 << QOC_MERGE_COL_BITS;
        std::vector<QocEllOp> ops(1);
        ops[0].len.assign((size_t)n, 0);
        QocMergedOps out;
        if (qoc_ell_merge(n, ops, out, why)) { printf("ok %d\n", out.Wm); return 0; }
        printf("error: %s\n", why.c_str());
        return 0;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int n = 0, K = 0;
    if (fscanf(f, "%d %d", &n, &K) != 2 || K < 0) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<QocEllOp> ops((size_t)K);
    for (int j = 0; j < K; ++j) {
        long long count = 0;
        if (fscanf(f, "%lld", &count) != 1 || count < 0) { fprintf(stderr, "bad count\n"); return 2; }
        std::vector<int32_t> row((size_t)count), col((size_t)count);
        std::vector<double> val(2 * (size_t)count);
        for (long long i = 0; i < count; ++i)
            if (fscanf(f, "%d %d %lf %lf", &row[(size_t)i], &col[(size_t)i], &val[2 * (size_t)i], &val[2 * (size_t)i + 1]) != 4) { fprintf(stderr, "bad entry\n"); return 2; }
        if (!qoc_ell_build(n, count, row.data(), col.data(), val.data(), ops[(size_t)j], why)) { printf("error: operator %d: %s\n", j, why.c_str()); fclose(f); return 0; }
    }
    fclose(f);
    QocMergedOps out;
    if (!qoc_ell_merge(n, ops, out, why)) { printf("error: %s\n", why.c_str()); return 0; }
    printf("ok %d\n", out.Wm);
    for (int r = 0; r < n; ++r) printf("%d\n", (int)out.len[(size_t)r]);
    for (size_t i = 0; i < (size_t)n * out.Wm; ++i)
        printf("%d %d %.17g %.17g\n", qoc_merge_col(out.idx[i]), qoc_merge_op(out.idx[i]), out.val[2 * i], out.val[2 * i + 1]);
    return 0;
}
