// qoc_sparse_host.h -- host side of the sparse state-transfer path: COO / CSR entries -> ELLPACK, slot-major.  No HIP dependency: plain C++,
// so that the builder compiles alone (tests/sparse_host_main.cpp runs it under the address and undefined-behaviour sanitizers).
//
// One operator at a time.  Input: `count` entries (row, col, complex value) in any order; duplicates of a position are summed in input order,
// explicit zeros are kept as stored entries.  Output: width W = the largest number of distinct columns in a row, and
//     col[slot * n + r], val[slot * n + r]     slot < W, r < n
// with the entries of a row in ascending column order and the padding slots pointing at the row itself with value 0 (a gather that is always
// in bounds and adds an exact zero).  An operator without entries has W = 0.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

struct QocEllOp {
    int W = 0;
    long long stored = 0;            // entries after the duplicates are merged (padding not counted)
    std::vector<int32_t> col;        // [W][n]
    std::vector<double> val;         // [W][n] complex, interleaved (re, im)
    std::vector<int32_t> len;        // [n] stored entries of row r: its first len[r] slots (the rest is padding)
};

// Returns true, or false with `why` naming the cause (an index outside 0 .. n-1, a non-finite value, n * W past int32).
static inline bool qoc_ell_build(int n, long long count, const int32_t* row, const int32_t* col, const double* val, QocEllOp& out, std::string& why) {
    char buf[160];
    out = QocEllOp();
    if (n < 1 || count < 0 || (count > 0 && (!row || !col || !val))) { why = "bad operator arguments"; return false; }
    for (long long i = 0; i < count; ++i) {
        if (row[i] < 0 || row[i] >= n || col[i] < 0 || col[i] >= n) {
            snprintf(buf, sizeof buf, "entry %lld has index (%d, %d) outside 0 .. %d", i, (int)row[i], (int)col[i], n - 1);
            why = buf;
            return false;
        }
        if (!std::isfinite(val[2 * i]) || !std::isfinite(val[2 * i + 1])) {
            snprintf(buf, sizeof buf, "entry %lld at (%d, %d) is not finite", i, (int)row[i], (int)col[i]);
            why = buf;
            return false;
        }
    }
    // entries by (row, column); a stable sort keeps the duplicates of a position in input order, so their sum is reproducible
    std::vector<long long> order((size_t)count);
    std::iota(order.begin(), order.end(), 0LL);
    std::stable_sort(order.begin(), order.end(), [&](long long a, long long b) { return row[a] != row[b] ? row[a] < row[b] : col[a] < col[b]; });
    // pass 1: distinct positions per row -> the width
    std::vector<int32_t> fill((size_t)n, 0);
    for (long long i = 0; i < count; ++i) {
        const long long e = order[(size_t)i];
        if (i > 0) { const long long p = order[(size_t)i - 1]; if (row[p] == row[e] && col[p] == col[e]) continue; }
        fill[(size_t)row[e]] += 1;
        out.stored += 1;
    }
    int W = 0;
    for (int r = 0; r < n; ++r) W = std::max(W, (int)fill[(size_t)r]);
    if ((long long)n * W > (long long)INT32_MAX) {
        snprintf(buf, sizeof buf, "n * width = %d * %d does not fit 32-bit indices (a row with %d entries: not a sparse operator)", n, W, W);
        why = buf;
        return false;
    }
    out.W = W;
    out.col.resize((size_t)n * W);
    out.val.assign(2 * (size_t)n * W, 0.0);
    for (int s = 0; s < W; ++s)
        for (int r = 0; r < n; ++r) out.col[(size_t)s * n + r] = r;          // padding: the row's own index, value 0
    // pass 2: the entries into their slots
    std::fill(fill.begin(), fill.end(), 0);
    for (long long i = 0; i < count; ++i) {
        const long long e = order[(size_t)i];
        const int r = row[e];
        bool dup = false;
        if (i > 0) { const long long p = order[(size_t)i - 1]; dup = row[p] == r && col[p] == col[e]; }
        if (!dup) fill[(size_t)r] += 1;
        const size_t at = (size_t)(fill[(size_t)r] - 1) * n + r;
        out.col[at] = col[e];
        out.val[2 * at] += val[2 * e];
        out.val[2 * at + 1] += val[2 * e + 1];
    }
    // a sum of finite duplicates may still overflow
    for (size_t i = 0; i < out.val.size(); ++i)
        if (!std::isfinite(out.val[i])) { why = "the sum of duplicate entries is not finite"; return false; }
    out.len = fill;
    return true;
}

// The merged layout of a list of operators (qoc_create_sparse_fleet, row_layout = 2): for every row ONE list that holds the stored entries of
// operator 0, then operator 1, and so on, in the slot order of each operator's own block (columns ascending); padding slots are dropped, explicit
// zeros stay.  A slot is the column and the operator index in one int32 (col | op << 24, read back as unsigned) and the complex value:
//     idx[slot * n + r], val[slot * n + r]     slot < Wm, r < n,   len[r] slots of row r in use
// Wm is the longest merged row; the slots behind len[r] hold the row's own index under operator 0 and value 0 and are never read.
#define QOC_MERGE_MAX_OPS 255
#define QOC_MERGE_COL_BITS 24
struct QocMergedOps {
    int Wm = 0;
    std::vector<int32_t> idx;        // [Wm][n]
    std::vector<double> val;         // [Wm][n] complex, interleaved (re, im)
    std::vector<int32_t> len;        // [n]
};
static inline int32_t qoc_merge_pack(int col, int op) { return (int32_t)((uint32_t)col | ((uint32_t)op << QOC_MERGE_COL_BITS)); }
static inline int qoc_merge_col(int32_t packed) { return (int)((uint32_t)packed & ((1u << QOC_MERGE_COL_BITS) - 1u)); }
static inline int qoc_merge_op(int32_t packed) { return (int)((uint32_t)packed >> QOC_MERGE_COL_BITS); }

// Returns true, or false with `why` naming the cause (too many operators, n past the packed column, a block that is not of this n, n * Wm past int32).
static inline bool qoc_ell_merge(int n, const std::vector<QocEllOp>& ops, QocMergedOps& out, std::string& why) {
    char buf[160];
    out = QocMergedOps();
    if (n < 1) { why = "bad operator arguments"; return false; }
    if (ops.size() > (size_t)QOC_MERGE_MAX_OPS) {
        snprintf(buf, sizeof buf, "%zu operators (the merged layout packs the operator index into 8 bits: at most %d)", ops.size(), QOC_MERGE_MAX_OPS);
        why = buf;
        return false;
    }
    if ((long long)n >= (1LL << QOC_MERGE_COL_BITS)) {
        snprintf(buf, sizeof buf, "n = %d (the merged layout packs the column into %d bits: n < %d)", n, QOC_MERGE_COL_BITS, 1 << QOC_MERGE_COL_BITS);
        why = buf;
        return false;
    }
    for (size_t j = 0; j < ops.size(); ++j) {
        const QocEllOp& o = ops[j];
        if (o.W < 0 || o.len.size() != (size_t)n || o.col.size() != (size_t)n * o.W || o.val.size() != 2 * (size_t)n * o.W) {
            snprintf(buf, sizeof buf, "operator %zu is not an ELLPACK block of n = %d", j, n);
            why = buf;
            return false;
        }
    }
    out.len.assign((size_t)n, 0);
    long long Wm = 0;
    for (int r = 0; r < n; ++r) {
        long long l = 0;
        for (const QocEllOp& o : ops) l += o.len[(size_t)r];
        Wm = std::max(Wm, l);
        if (l <= (long long)INT32_MAX) out.len[(size_t)r] = (int32_t)l;
    }
    if ((long long)n * Wm > (long long)INT32_MAX) {
        snprintf(buf, sizeof buf, "n * merged width = %d * %lld does not fit 32-bit indices", n, Wm);
        why = buf;
        return false;
    }
    out.Wm = (int)Wm;
    out.idx.resize((size_t)n * out.Wm);
    out.val.assign(2 * (size_t)n * out.Wm, 0.0);
    for (int s = 0; s < out.Wm; ++s)
        for (int r = 0; r < n; ++r) out.idx[(size_t)s * n + r] = qoc_merge_pack(r, 0);
    std::vector<int32_t> fill((size_t)n, 0);
    for (size_t j = 0; j < ops.size(); ++j) {
        const QocEllOp& o = ops[j];
        for (int s = 0; s < o.W; ++s)
            for (int r = 0; r < n; ++r) {
                if (s >= o.len[(size_t)r]) continue;
                const size_t from = (size_t)s * n + r, at = (size_t)fill[(size_t)r] * n + r;
                fill[(size_t)r] += 1;
                out.idx[at] = qoc_merge_pack(o.col[from], (int)j);
                out.val[2 * at] = o.val[2 * from];
                out.val[2 * at + 1] = o.val[2 * from + 1];
            }
    }
    return true;
}
