// qoc_ensemble.h -- robust GRAPE: one pulse per control set, optimised for the weighted mean objective over E members.
//
// Member e of an ensemble has the drift H0 + sum_q delta[e][q] P_q and the controls a[e][j] H_j.  The engine holds it as trajectories of
// ONE shared stack [H0, H_1 .. H_k, P_1 .. P_q] with k' = k + q controls: trajectory (g, e) = g E + e runs u_j = a[e][j] maxA_j sin(base_g[j])
// for j < k and the frozen rows u_{k+q'} = delta[e][q'], so every forward / loss / backward kernel runs on the trajectories unchanged.  The
// per-control-set state (base, Adam slots, stop rule, pulse regularisers) lives in a second QocDev view of G rows and k controls, on which the
// existing tails run unchanged.  The two kernels below are the glue between the views: plain loads, stores and a fixed summation order (no
// atomics), so a run is bit-reproducible, and an ensemble of one nominal member (E = 1, q = 0, a = 1, w = 1) computes exactly what the
// plain engine computes.
#pragma once
#include "qoc_common.h"

struct QocEns {
    int E, q;
    const double* a;       // [E][k]  amplitude scale of each control
    const double* delta;   // [E][q]  value of each frozen perturbation row
    const double* wt;      // [E]     member weights
};

// Trajectory controls from the group's: thread per (group, row j < k', slice), a loop over the members.  from_base: the group's controls
// are formed here from its variable (w = sin(base), u = maxA w: k_controls' arithmetic) and stored to the group view too; else they are the
// group's u (what the Adam tail left in u2 and the engine swapped in).  Also mirrors the group's done flag into its trajectories: the heavy
// kernels skip finished trajectories by their own flag.
__global__ void __launch_bounds__(256) k_ens_expand(QocDev t, QocDev g, QocEns en, int from_base) {
    const int steps = g.steps, k = g.k, kp = t.k, E = en.E;
    const size_t total = (size_t)g.B * kp * steps;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int tt = (int)(i % steps);
        const int j = (int)((i / steps) % kp);
        const int gi = (int)(i / ((size_t)steps * kp));
        double* tu = t.u + ((size_t)gi * E * kp + j) * steps + tt;
        const size_t tstride = (size_t)kp * steps;
        if (j < k) {
            const size_t go = ((size_t)gi * k + j) * steps + tt;
            double gu;
            if (from_base) {
                const double w = sin(g.base[go]);
                gu = g.maxA[j] * w;
                g.w[go] = w;
                g.u[go] = gu;
            } else {
                gu = g.u[go];
            }
            for (int e = 0; e < E; ++e) tu[(size_t)e * tstride] = en.a[(size_t)e * k + j] * gu;
        } else {
            for (int e = 0; e < E; ++e) tu[(size_t)e * tstride] = en.delta[(size_t)e * en.q + (j - k)];
        }
        if (j == 0 && tt == 0)
            for (int e = 0; e < E; ++e) t.done[(size_t)gi * E + e] = g.done[gi];
    }
}

// Group gradient and scalars from the members': dLdu_g[j][t] = sum_e (w_e a[e][j]) dLdu_(g,e)[j][t] for j < k, loss_g and reg_state_g the
// weighted sums of the members' (which stay readable in the trajectory arrays).  Grid (ceil(k steps / 256), G); members summed in the order
// 0 .. E-1, starting from member 0's term.  A finished group of a loop iteration is left alone (its members were not re-evaluated).
__global__ void __launch_bounds__(256) k_ens_reduce(QocDev t, QocDev g, QocEns en) {
#pragma clang fp contract(off)
    const int gi = blockIdx.y;
    if (g.skip_done && g.done[gi]) return;
    const int steps = g.steps, k = g.k, kp = t.k, E = en.E, ks = k * steps;
    const size_t tstride = (size_t)kp * steps;
    const double* src = t.dLdu + (size_t)gi * E * tstride;
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o < ks) {
        const int j = o / steps;
        double acc = (en.wt[0] * en.a[j]) * src[o];
        for (int e = 1; e < E; ++e) acc = acc + (en.wt[e] * en.a[(size_t)e * k + j]) * src[(size_t)e * tstride + o];
        g.dLdu[(size_t)gi * ks + o] = acc;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const size_t b0 = (size_t)gi * E;
        double l = en.wt[0] * t.loss[b0], r = en.wt[0] * t.reg_state[b0];
        for (int e = 1; e < E; ++e) { l = l + en.wt[e] * t.loss[b0 + e]; r = r + en.wt[e] * t.reg_state[b0 + e]; }
        g.loss[gi] = l;
        g.reg_state[gi] = r;
    }
}
