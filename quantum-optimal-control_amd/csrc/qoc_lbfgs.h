// qoc_lbfgs.h -- the step of the device-resident L-BFGS loop (qoc_iterate_lbfgs / qoc_run_lbfgs).
//
// One loop iteration is an evaluate-only iteration (the mode-0 tail leaves base, grad, reg_loss = the objective f, loss and grad_squared of every
// control set) followed by ONE launch of k_lbfgs_step: one workgroup per control set takes the stop rule, the Armijo test of the trial point,
// and either accepts it (new curvature pair, new direction, first trial of the next search) or shrinks the step.  Every control set has its own
// history, direction, step length and flags; nothing is shared between sets, and every sum is taken in a fixed order.
//
// The direction is built in the Gram form.  With M pairs the plain two-loop recursion is 2M + 3 dependent workgroup reductions of two barriers
// each; here the (2M + 1)^2 dot products among [S_0 .. S_{M-1}, Y_0 .. Y_{M-1}, g] are kept per control set, an accepted step forms the dots of
// the new s, y and g with the stored vectors while it streams them once (pass 1, in sub-passes of QOC_LBFGS_COLS stored vectors so that the
// accumulators fit the registers of a 1024-thread launch), ONE multi-value reduction sums them, one lane runs the recursion on the 2M + 1
// coefficients, and a second pass forms p as their linear combination while it stores the new pair, the accepted point and the next trial.
// The number of barriers of a step is 5, whatever M.
#pragma once

#include "qoc_common.h"

#define QOC_LBFGS_MAX_M 16                              // pairs kept at most (qoc_lbfgs_params.history)
#define QOC_LBFGS_COLS 8                                // stored vectors per sub-pass of pass 1: 3 x 8 fp64 accumulators per thread
#define QOC_LBFGS_ROWS (2 * QOC_LBFGS_MAX_M + 1)        // vectors of the Gram matrix at most
#define QOC_LBFGS_VALS (6 * QOC_LBFGS_MAX_M + 6)        // values of pass 1 at most: (s, y, g) . each stored vector, ss, sy, yy, gs, gy, gg
#define QOC_LBFGS_WAVES 16

// per-set state: st[8] = {started, restoring, count, head, ls, 0, 0, 0}; sc[4] = {f_acc, alpha, gp, 0}
struct QocLbfgsDev {
    double* vec;        // [B][2M + 3][N]: x_acc, g_acc, p, S[M], Y[M]
    double* gram;       // [B][2M + 1][2M + 1] dots among S (rows 0 .. M-1), Y (rows M .. 2M-1) and g_acc (row 2M); only rows of live slots are read
    double* sc;         // [B][4]
    int* st;            // [B][8]
    int M, N;           // pairs kept; elements of a control set (k steps, or k P samples)
    double conv_target, min_grad, c1, shrink;
    int max_iterations, max_ls;
};

// the wave's sum of v in lane 0 (fixed order)
__device__ __forceinline__ double lbfgs_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__global__ void __launch_bounds__(1024) k_lbfgs_step(QocDev d, QocLbfgsDev L) {
    // no implicit contraction into FMAs: the Armijo test and the trial points round as the plain expressions do (tests/lbfgs_reference.py)
#pragma clang fp contract(off)
    __shared__ double part[QOC_LBFGS_VALS * QOC_LBFGS_WAVES];      // [value][wave] partial sums of pass 1
    __shared__ double dots[QOC_LBFGS_VALS];
    __shared__ double G[QOC_LBFGS_ROWS * QOC_LBFGS_ROWS];
    __shared__ double coef[QOC_LBFGS_ROWS];                        // p = sum coef[j] vector_j
    __shared__ double aa[QOC_LBFGS_MAX_M];                         // the a_i of the recursion
    __shared__ double outd[2];                                     // gp of the new direction
    __shared__ int outi[4];                                        // count, head after the step; slot written (-1: none)
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wid = tid >> 6, nw = (nt + 63) >> 6;
    const int N = L.N, M = L.M, R = 2 * M + 1;
    const bool writer = tid == 0;
    if (d.done[b]) return;
    int* st = L.st + (size_t)b * 8;
    double* sc = L.sc + (size_t)b * 4;
    double* gram = L.gram + (size_t)b * R * R;
    double* base = d.base + (size_t)b * N;
    const double* grad = d.grad + (size_t)b * N;
    double* xacc = L.vec + (size_t)b * (2 * M + 3) * N;
    double* gacc = xacc + N;
    double* p = gacc + N;
    double* S = p + N;
    double* Y = S + (size_t)M * N;
    const int started = st[0], restoring = st[1], count = st[2], head = st[3];
    int ls = st[4];
    const double f = d.reg_loss[b], loss = d.loss[b], g2 = d.g2[b];
    const double f_acc = sc[0], gp = sc[2];
    double alpha = sc[1];
    const int it0 = d.iters[b];
    __syncthreads();                                    // every thread holds the state before thread 0 rewrites it

    if (restoring) { if (writer) d.done[b] = 1; return; }                       // this evaluation was of the accepted point
    if (loss < L.conv_target || g2 < L.min_grad) { if (writer) d.done[b] = 1; return; }
    const bool acceptable = !started || (isfinite(f) && f <= f_acc + L.c1 * alpha * gp);
    if (it0 >= L.max_iterations) {
        if (acceptable) { if (writer) d.done[b] = 1; return; }
        for (int o = tid; o < N; o += nt) base[o] = xacc[o];
        if (writer) st[1] = 1;
        return;
    }
    if (writer) d.iters[b] = it0 + 1;

    if (!acceptable) {                                  // ---- reject: shrink the step, or give the direction up
        ls += 1;
        if (ls > L.max_ls) {
            if (count == 0) {                           // steepest descent stalled too: back to the accepted point, one evaluation there, done
                for (int o = tid; o < N; o += nt) base[o] = xacc[o];
                if (writer) st[1] = 1;
                return;
            }
            const double gg = gram[(size_t)(R - 1) * R + (R - 1)], nrm = sqrt(gg);
            alpha = 1.0 / L.shrink;
            alpha *= L.shrink;
            for (int o = tid; o < N; o += nt) {
                const double pv = -(gacc[o] / nrm);
                p[o] = pv;
                base[o] = xacc[o] + alpha * pv;
            }
            if (writer) { sc[1] = alpha; sc[2] = -(gg / nrm); st[2] = 0; st[3] = 0; st[4] = 0; }
            return;
        }
        alpha *= L.shrink;
        for (int o = tid; o < N; o += nt) base[o] = xacc[o] + alpha * p[o];
        if (writer) { sc[1] = alpha; st[4] = ls; }
        return;
    }

    // ---- accept.  Pass 1: the dots of s = x - x_acc, y = g - g_acc and g with the 2 count stored vectors (compact index i: S_i, then Y_{i - count};
    // the live slots are 0 .. count - 1), value 3 i + {0: s, 1: y, 2: g}, then ss, sy, yy, gs, gy, gg
    const int nv = 2 * count, nvals = 3 * nv + 6;
    for (int c0 = 0; c0 < nv; c0 += QOC_LBFGS_COLS) {
        const double* vp[QOC_LBFGS_COLS];
#pragma unroll
        for (int j = 0; j < QOC_LBFGS_COLS; ++j) {
            const int i = c0 + j < nv ? c0 + j : c0;                            // past the end: a live vector again, its sums are dropped
            vp[j] = i < count ? S + (size_t)i * N : Y + (size_t)(i - count) * N;
        }
        double acc[QOC_LBFGS_COLS][3];
#pragma unroll
        for (int j = 0; j < QOC_LBFGS_COLS; ++j) { acc[j][0] = 0.0; acc[j][1] = 0.0; acc[j][2] = 0.0; }
        for (int o = tid; o < N; o += nt) {
            const double gv = grad[o], sv = base[o] - xacc[o], yv = gv - gacc[o];
#pragma unroll
            for (int j = 0; j < QOC_LBFGS_COLS; ++j) {
                const double v = vp[j][o];
                acc[j][0] += sv * v; acc[j][1] += yv * v; acc[j][2] += gv * v;
            }
        }
#pragma unroll
        for (int j = 0; j < QOC_LBFGS_COLS; ++j) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double t = lbfgs_wave_sum(acc[j][a]);
                if (lane == 0 && c0 + j < nv) part[(3 * (c0 + j) + a) * QOC_LBFGS_WAVES + wid] = t;
            }
        }
    }
    {
        double e[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int o = tid; o < N; o += nt) {
            const double gv = grad[o], sv = started ? base[o] - xacc[o] : 0.0, yv = started ? gv - gacc[o] : 0.0;
            e[0] += sv * sv; e[1] += sv * yv; e[2] += yv * yv; e[3] += gv * sv; e[4] += gv * yv; e[5] += gv * gv;
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const double t = lbfgs_wave_sum(e[a]);
            if (lane == 0) part[(3 * nv + a) * QOC_LBFGS_WAVES + wid] = t;
        }
    }
    for (int o = tid; o < R * R; o += nt) G[o] = gram[o];
    __syncthreads();
    if (tid < nvals) {
        double t = 0.0;
        for (int w = 0; w < nw; ++w) t += part[tid * QOC_LBFGS_WAVES + w];
        dots[tid] = t;
    }
    __syncthreads();

    // the new pair enters slot h when its curvature is positive enough, in place of the oldest pair of a full history
    const double ss = dots[3 * nv], sy = dots[3 * nv + 1], yy = dots[3 * nv + 2], gs = dots[3 * nv + 3], gy = dots[3 * nv + 4], gg = dots[3 * nv + 5];
    const bool push = started && sy > 1e-10 * yy;
    const int h = head;
    if (tid < 2 * M) {                                  // row / column tid of the Gram matrix
        const int q = tid, slot = q < M ? q : q - M;
        const int ci = q < M ? q : count + (q - M);     // its compact index in pass 1 (live slots only)
        if (push && slot == h) {
            if (q < M) {
                G[q * R + q] = ss; G[q * R + (q + M)] = sy; G[(q + M) * R + q] = sy;
                G[q * R + 2 * M] = gs; G[2 * M * R + q] = gs;
            } else {
                G[q * R + q] = yy;
                G[q * R + 2 * M] = gy; G[2 * M * R + q] = gy;
            }
        } else if (slot < count) {
            if (push) {
                G[h * R + q] = dots[3 * ci]; G[q * R + h] = dots[3 * ci];
                G[(h + M) * R + q] = dots[3 * ci + 1]; G[q * R + (h + M)] = dots[3 * ci + 1];
            }
            G[2 * M * R + q] = dots[3 * ci + 2]; G[q * R + 2 * M] = dots[3 * ci + 2];
        }
    } else if (tid == 2 * M) G[2 * M * R + 2 * M] = gg;
    __syncthreads();

    if (writer) {                                       // the two-loop recursion on coefficients: q = g, r = gamma q + ..., p = -r
        int cnt = count, hd = head;
        if (push) { cnt = count < M ? count + 1 : M; hd = h + 1 == M ? 0 : h + 1; }
        for (int j = 0; j < R; ++j) coef[j] = 0.0;
        coef[2 * M] = 1.0;
        const int newest = hd == 0 ? M - 1 : hd - 1;    // (cnt > 0; with cnt < M the live slots are 0 .. cnt - 1 and hd = cnt)
        // v_row . (sum_j coef_j vector_j) over the live vectors, in a fixed order
        auto dot_row = [&](int row) {
            double t = coef[2 * M] * G[row * R + 2 * M];
            for (int j = 0; j < cnt; ++j) { t += coef[j] * G[row * R + j]; t += coef[M + j] * G[row * R + M + j]; }
            return t;
        };
        if (cnt > 0) {
            int i = newest;
            for (int t = 0; t < cnt; ++t) {
                const double a = dot_row(i) / G[i * R + M + i];
                aa[i] = a;
                coef[M + i] -= a;
                i = i == 0 ? M - 1 : i - 1;
            }
            const double gamma = G[newest * R + M + newest] / G[(M + newest) * R + M + newest];
            coef[2 * M] *= gamma;
            for (int j = 0; j < cnt; ++j) { coef[j] *= gamma; coef[M + j] *= gamma; }
            i = cnt == M ? hd : 0;                      // the oldest
            for (int t = 0; t < cnt; ++t) {
                const double beta = dot_row(M + i) / G[i * R + M + i];
                coef[i] += aa[i] - beta;
                i = i + 1 == M ? 0 : i + 1;
            }
        }
        double gpn = 0.0;
        if (cnt > 0) gpn = -dot_row(2 * M);
        if (cnt == 0 || !(gpn < 0.0)) {                 // no history, or not a descent direction: steepest descent of unit length
            const double nrm = sqrt(gg);
            for (int j = 0; j < R; ++j) coef[j] = 0.0;
            coef[2 * M] = 1.0 / nrm;
            gpn = -(gg / nrm);
            cnt = 0; hd = 0;
        }
        for (int j = 0; j < R; ++j) coef[j] = -coef[j];
        outd[0] = gpn;
        outi[0] = cnt; outi[1] = hd; outi[2] = push ? h : -1;
    }
    __syncthreads();

    // ---- pass 2: the new pair into its slot, the accepted point, p and the first trial of the search along it
    const int cnt = outi[0], hnew = outi[2];
    const bool steepest = cnt == 0;                     // p = -(g / |g|), as a rejected search falls back to it
    const double cg = coef[2 * M];
    for (int o = tid; o < N; o += nt) {
        const double xv = base[o], gv = grad[o];
        const double sv = xv - xacc[o], yv = gv - gacc[o];
        double pv = steepest ? -(gv / sqrt(gg)) : cg * gv;
        for (int j = 0; j < cnt; ++j) {
            const double sj = j == hnew ? sv : S[(size_t)j * N + o], yj = j == hnew ? yv : Y[(size_t)j * N + o];
            pv += coef[j] * sj;
            pv += coef[M + j] * yj;
        }
        if (hnew >= 0) { S[(size_t)hnew * N + o] = sv; Y[(size_t)hnew * N + o] = yv; }
        xacc[o] = xv; gacc[o] = gv; p[o] = pv;
        base[o] = xv + pv;
    }
    for (int o = tid; o < R * R; o += nt) gram[o] = G[o];
    if (writer) {
        sc[0] = f; sc[1] = 1.0; sc[2] = outd[0];
        st[0] = 1; st[2] = cnt; st[3] = outi[1]; st[4] = 0;
    }
}
