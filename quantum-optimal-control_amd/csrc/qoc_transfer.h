// qoc_transfer.h -- transfer-function GRAPE: the variable is the P samples per line an AWG plays, the pulse the Hamiltonian sees is a known
// linear response of them.
//
// T is a real steps x P matrix (zero-order hold, interpolation, a filter or line response).  Control set g has the variable theta_g [k][P]:
// w_s = sin(theta_g) and u_s = maxA_j w_s are the samples, w_f[j][t] = sum_p T[t][p] w_s[j][p] and u_f = maxA_j w_f is the pulse every
// trajectory of the control set runs on (member e of an ensemble: a[e][j] u_f and its frozen perturbation rows).  It is the cut of
// qoc_ensemble.h with a matrix in it: the trajectory view (G E trajectories, k + q controls, `steps` slices) runs every forward / loss /
// backward kernel unchanged, the sample view (G control sets, k controls, P "slices" of total_time / P) holds the variable, Adam, the stop
// rule and the pulse regularisers, and the existing tails run on it unchanged.  The two kernels below replace k_ens_expand / k_ens_reduce:
// T on the way down, T^T on the way up (both from the transposed copy the host uploads).  Hold, interpolation and FIR responses are banded, so both loop over the nonzero window of their
// row / column only (found on the host at create time).  Plain loads, stores and a fixed summation order (no atomics, no contraction): a
// run is bit-reproducible, and the identity response with one nominal member computes exactly what the plain engine computes.
#pragma once
#include "qoc_common.h"
#include "qoc_ensemble.h"

struct QocShape {
    int P;                 // samples per line
    int band;              // widest row window
    int col_band;          // widest column window
    const double* Tt;      // [P][steps]: T transposed, the only copy on the device -- both kernels run over neighbouring slices in neighbouring
                           // threads, so both read it along its rows (reading T itself in k_shape_expand: 57 us instead of 27 for a dense 500 x 125
                           // T at 64 control sets of 4 controls, no difference for banded ones; profiles/transfer_overhead.txt)
    const int2* row_win;   // [steps]  [lo, hi): the nonzero entries of row t lie in it (lo = hi: an all-zero row)
    const int2* col_win;   // [P]      [tlo, thi) of column p
    double* uf;            // [G][k][steps] the nominal pulse u_f of the last evaluation (qoc_get_pulse)
};

// column windows up to this many slices: one thread per output; longer ones (a dense T): one wave per output
#define QOC_SHAPE_WAVE_FROM 32

// Trajectory controls from the samples: thread per (control set, row j < k', slice t).  s.w holds w_s of the evaluation (k_controls on the
// sample view, or what the Adam tail left and the engine swapped in): no sin here.  The row window is summed in ascending p, starting from
// its first term.  Stores the nominal pulse, every member's scaled copy and the frozen perturbation rows, and mirrors the done flags
// (as k_ens_expand).  TRACES (k_shape_expand_traces, launched while a table is set): a frozen row is delta[e][q'] + tr[e][q'][t], as in
// k_ens_expand_traces; k_shape_expand itself is the code it was before the table existed.
template <bool TRACES>
__device__ __forceinline__ void shape_expand_body(const QocDev& t, const QocDev& s, const QocEns& en, const QocShape& sh) {
#pragma clang fp contract(off)
    const int steps = t.steps, P = sh.P, k = s.k, kp = t.k, E = en.E;
    const size_t total = (size_t)s.B * kp * steps;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int tt = (int)(i % steps);
        const int j = (int)((i / steps) % kp);
        const int gi = (int)(i / ((size_t)steps * kp));
        double* tu = t.u + ((size_t)gi * E * kp + j) * steps + tt;
        const size_t tstride = (size_t)kp * steps;
        const size_t dev = (size_t)(gi / en.R) * E;                  // the first member row of this control set's device
        if (j < k) {
            // (row tt of T from the transposed copy: neighbouring threads are neighbouring slices, whose windows overlap)
            const int2 win = sh.row_win[tt];
            const double* row = sh.Tt + tt;
            const double* ws = s.w + ((size_t)gi * k + j) * P;
            double wf = 0.0;
            if (win.x < win.y) {
                wf = row[(size_t)win.x * steps] * ws[win.x];
                for (int p = win.x + 1; p < win.y; ++p) wf = wf + row[(size_t)p * steps] * ws[p];
            }
            const double gu = s.maxA[j] * wf;
            sh.uf[((size_t)gi * k + j) * steps + tt] = gu;
            const double* a = en.a + dev * k;
            for (int e = 0; e < E; ++e) tu[(size_t)e * tstride] = a[(size_t)e * k + j] * gu;
        } else {
            const double* delta = en.delta + dev * en.q;
            if (TRACES) {
                const size_t estride = (size_t)en.q * steps;
                const double* tr = en.tr + (dev * en.q + (j - k)) * steps + tt;
                ens_trace_rows(tu, tstride, delta + (j - k), en.q, tr, estride, E);
            } else {
                for (int e = 0; e < E; ++e) tu[(size_t)e * tstride] = delta[(size_t)e * en.q + (j - k)];
            }
        }
        if (j == 0 && tt == 0)
            for (int e = 0; e < E; ++e) t.done[(size_t)gi * E + e] = s.done[gi];
    }
}
__global__ void __launch_bounds__(256) k_shape_expand(QocDev t, QocDev s, QocEns en, QocShape sh) { shape_expand_body<false>(t, s, en, sh); }
__global__ void __launch_bounds__(256) k_shape_expand_traces(QocDev t, QocDev s, QocEns en, QocShape sh) { shape_expand_body<true>(t, s, en, sh); }

// the members' weighted gradient of one (j, t) element: members summed 0 .. E-1 from member 0's term (k_ens_reduce's arithmetic); a: the
// amplitude rows of the control set's device
__device__ __forceinline__ double shape_member_sum(const double* __restrict__ src, const QocEns& en, const double* __restrict__ a, int j, int k,
                                                   size_t tstride) {
#pragma clang fp contract(off)
    double acc = (en.wt[0] * a[j]) * src[0];
    for (int e = 1; e < en.E; ++e) acc = acc + (en.wt[e] * a[(size_t)e * k + j]) * src[(size_t)e * tstride];
    return acc;
}

// Sample gradient and scalars from the trajectories': dLdu_s[g][j][p] = sum_t T[t][p] sum_e (w_e a[e][j]) dLdu_(g,e)[j][t], loss_g and
// reg_state_g the weighted sums of the members'.  Grid (ceil(k P / (256 / LANES)), G).  LANES = 1: one thread per output, the column window
// in ascending t from its first term.  LANES = 64: one wave per output -- lane l sums t = tlo + l, tlo + l + 64, .. in ascending order, then a
// butterfly over the lanes (a fixed order: the result does not depend on the launch).  The column of T is read from the transposed copy:
// consecutive t at consecutive addresses.  A finished control set of a loop iteration is left alone.
template <int LANES>
__global__ void __launch_bounds__(256) k_shape_reduce(QocDev t, QocDev s, QocEns en, QocShape sh) {
#pragma clang fp contract(off)
    const int gi = blockIdx.y;
    if (s.skip_done && s.done[gi]) return;
    const int steps = t.steps, P = sh.P, k = s.k, kp = t.k, E = en.E, kP = k * P;
    const size_t tstride = (size_t)kp * steps;
    const int o = (int)((blockIdx.x * blockDim.x + threadIdx.x) / LANES), lane = threadIdx.x % LANES;
    if (o < kP) {                                   // (LANES = 64: uniform over the wave)
        const int j = o / P, p = o % P;
        const int2 win = sh.col_win[p];
        const double* col = sh.Tt + (size_t)p * steps;
        const double* src = t.dLdu + (size_t)gi * E * tstride + (size_t)j * steps;
        const double* a = en.a + (size_t)(gi / en.R) * E * k;
        double acc = 0.0;
        int tt = win.x + lane;
        if (tt < win.y) {
            acc = col[tt] * shape_member_sum(src + tt, en, a, j, k, tstride);
            for (tt += LANES; tt < win.y; tt += LANES) acc = acc + col[tt] * shape_member_sum(src + tt, en, a, j, k, tstride);
        }
        if (LANES > 1) {
#pragma unroll
            for (int off = LANES / 2; off > 0; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
        }
        if (lane == 0) s.dLdu[(size_t)gi * kP + o] = acc;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const size_t b0 = (size_t)gi * E;
        double l = en.wt[0] * t.loss[b0], r = en.wt[0] * t.reg_state[b0];
        for (int e = 1; e < E; ++e) { l = l + en.wt[e] * t.loss[b0 + e]; r = r + en.wt[e] * t.reg_state[b0 + e]; }
        s.loss[gi] = l;
        s.reg_state[gi] = r;
    }
}

// k_shape_reduce with the control set's tilted weights (k_ens_tilt, csrc/qoc_ensemble.h) where that reads en.wt: same grids, same orders of
// members, slices and lanes; the scalars are k_ens_tilt's.
template <int LANES>
__global__ void __launch_bounds__(256) k_shape_reduce_risk(QocDev t, QocDev s, QocEns en, QocShape sh, const double* __restrict__ pi_all) {
#pragma clang fp contract(off)
    const int gi = blockIdx.y;
    if (s.skip_done && s.done[gi]) return;
    const int steps = t.steps, P = sh.P, k = s.k, kp = t.k, E = en.E, kP = k * P;
    const size_t tstride = (size_t)kp * steps;
    QocEns er = en;
    er.wt = pi_all + (size_t)gi * E;
    const int o = (int)((blockIdx.x * blockDim.x + threadIdx.x) / LANES), lane = threadIdx.x % LANES;
    if (o < kP) {                                   // (LANES = 64: uniform over the wave)
        const int j = o / P, p = o % P;
        const int2 win = sh.col_win[p];
        const double* col = sh.Tt + (size_t)p * steps;
        const double* src = t.dLdu + (size_t)gi * E * tstride + (size_t)j * steps;
        const double* a = en.a + (size_t)(gi / en.R) * E * k;
        double acc = 0.0;
        int tt = win.x + lane;
        if (tt < win.y) {
            acc = col[tt] * shape_member_sum(src + tt, er, a, j, k, tstride);
            for (tt += LANES; tt < win.y; tt += LANES) acc = acc + col[tt] * shape_member_sum(src + tt, er, a, j, k, tstride);
        }
        if (LANES > 1) {
#pragma unroll
            for (int off = LANES / 2; off > 0; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
        }
        if (lane == 0) s.dLdu[(size_t)gi * kP + o] = acc;
    }
}
