// qoc_control_map.h -- control maps: the coefficients of the Hamiltonian as functions of the pulses.
//
// Every trajectory kernel runs H(t) = H0 + sum_i c_i[t] G_i on a generic stack of operators with one coefficient row each.  Without a map
// the rows ARE the member's pulses v_j[t] = a[e][j] u_g[j][t] (qoc_ensemble.h; the filtered u_f of qoc_transfer.h).  With a map, for the r
// operators the map feeds and the k pulses,
//   c_i[t] = F[i][t] + sum_{j < k} M[i][j][t] p_ij(v_j[t]),      p_ij(x) = sum_{d = 1 .. D} alpha[i][j][d] x^d
// (M absent: ones; F absent: zeros; r need not equal k), and the member's q frozen perturbation rows follow as they are.  The map is one more
// stage of the glue between the views: the member glue (k_ens_expand / k_shape_expand, k_ens_reduce / k_shape_reduce and their _risk forms)
// reads and writes a PULSE view -- a copy of the trajectory view with k + q rows whose u / dLdu are two staging arrays [G E][k + q][steps]
// and whose loss, reg_state and done are the trajectories' own -- and the two kernels below join the pulse view and the trajectory view:
//   k_map_expand : c from v, after the member glue has written v
//   k_map_reduce : dJ/dv_j[t] = sum_i dJ/dc_i[t] M[i][j][t] p_ij'(v_j[t]), after the backward kernels have left dJ/dc in the trajectories' dLdu
// No trajectory kernel, tail or optimiser changes.  Plain loads and stores, no atomics, no contraction, one fixed order of every sum (pulses j
// ascending from the first term, Horner from the highest power, operators i ascending from the first term): two evaluations agree bit for bit,
// and the identity map (r = k, D = 1, alpha = I, no M, no F) reproduces the engine without a map -- every product is by 1.0 or 0.0 and every
// added term a zero.
#pragma once
#include "qoc_common.h"

#define QOC_MAP_MAX_DEGREE 8
#define QOC_MAP_MAX_TERMS 64

struct QocMap {
    int r, D;              // operators fed, degree of the polynomials
    int k, q;              // pulses, frozen perturbation rows of a member
    const double* alpha;   // [r][k][D]      powers 1 .. D
    const double* M;       // [r][k][steps]  or null (ones)
    const double* F;       // [r][steps]     or null (zeros)
};

// p(x) = x (a_1 + x (a_2 + .. x a_D)) of one (operator, pulse) pair, a = its D coefficients
__device__ __forceinline__ double map_poly(const double* __restrict__ a, int D, double x) {
#pragma clang fp contract(off)
    double h = a[D - 1];
    for (int d = D - 2; d >= 0; --d) h = a[d] + x * h;
    return x * h;
}
// p'(x) = a_1 + x (2 a_2 + x (3 a_3 + .. x D a_D))
__device__ __forceinline__ double map_dpoly(const double* __restrict__ a, int D, double x) {
#pragma clang fp contract(off)
    double h = (double)D * a[D - 1];
    for (int d = D - 2; d >= 0; --d) h = (double)(d + 1) * a[d] + x * h;
    return h;
}

// Trajectory coefficients from the members' pulses: thread per (trajectory, row i < r + q, slice), grid-stride.  t: the trajectory view
// (r + q rows), p: the pulse view (k + q rows).  A frozen row is copied through.
__global__ void __launch_bounds__(QOC_BLOCK) k_map_expand(QocDev t, QocDev p, QocMap mp) {
#pragma clang fp contract(off)
    const int steps = t.steps, r = mp.r, k = mp.k, D = mp.D, rows = r + mp.q, prows = k + mp.q;
    const size_t total = (size_t)t.B * rows * steps;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const int tt = (int)(o % steps);
        const int i = (int)((o / steps) % rows);
        const size_t b = o / ((size_t)steps * rows);
        const double* v = p.u + b * prows * steps + tt;              // v[j steps]: pulse j of this trajectory at this slice
        double c;
        if (i < r) {
            const double* a = mp.alpha + (size_t)i * k * D;
            const double* mx = mp.M ? mp.M + (size_t)i * k * steps + tt : nullptr;
            c = map_poly(a, D, v[0]);
            if (mx) c = mx[0] * c;
            for (int j = 1; j < k; ++j) {
                double term = map_poly(a + (size_t)j * D, D, v[(size_t)j * steps]);
                if (mx) term = mx[(size_t)j * steps] * term;
                c = c + term;
            }
            if (mp.F) c = mp.F[(size_t)i * steps + tt] + c;
        } else {
            c = v[(size_t)(k + (i - r)) * steps];
        }
        t.u[o] = c;
    }
}

// The members' pulse gradients from the trajectories' coefficient gradients: thread per (trajectory, pulse j < k, slice), grid-stride.  The
// rows of the frozen perturbations have no reader (the member reduction stops at k) and are not written.
__global__ void __launch_bounds__(QOC_BLOCK) k_map_reduce(QocDev t, QocDev p, QocMap mp) {
#pragma clang fp contract(off)
    const int steps = t.steps, r = mp.r, k = mp.k, D = mp.D, rows = r + mp.q, prows = k + mp.q;
    const size_t total = (size_t)t.B * k * steps;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const int tt = (int)(o % steps);
        const int j = (int)((o / steps) % k);
        const size_t b = o / ((size_t)steps * k);
        const size_t po = (b * prows + j) * steps + tt;
        const double x = p.u[po];
        const double* gc = t.dLdu + b * rows * steps + tt;           // gc[i steps]: dJ/dc_i of this trajectory at this slice
        const double* a = mp.alpha + (size_t)j * D;
        const double* mx = mp.M ? mp.M + (size_t)j * steps + tt : nullptr;
        double acc = 0.0;
        for (int i = 0; i < r; ++i) {
            double gi = gc[(size_t)i * steps];
            if (mx) gi = gi * mx[(size_t)i * k * steps];
            const double term = gi * map_dpoly(a + (size_t)i * k * D, D, x);
            acc = i == 0 ? term : acc + term;
        }
        p.dLdu[po] = acc;
    }
}
