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

// A fleet (qoc_create_fleet) has F devices with a member table each: control set g belongs to device g / R and reads the block (g / R) E k of a,
// (g / R) E q of delta.  The three older entry points make F = 1, R = the number of control sets: block 0 for every control set.
struct QocEns {
    int E, q;
    int R;                 // control sets per device
    const double* a;       // [F][E][k]  amplitude scale of each control
    const double* delta;   // [F][E][q]  value of each frozen perturbation row
    const double* wt;      // [E]        member weights
    const double* tr;      // [F][E][q][steps] noise traces (qoc_set_traces): frozen row q' of member e runs delta[e][q'] + tr[e][q'][t]; null: none
};

// One frozen row at one slice with a trace table, for the members 0 .. E-1 in that order: tu[e tstride] = delta[e q] + tr[e estride].  Eight
// members' loads are issued before their eight stores: the loop is a chain of independent loads `q steps` doubles apart, and one load per trip
// left a thread of the qubit x 1024-member ensemble waiting for each in turn (0.29 ms per iteration; profiles/noise_traces.txt).  The values and
// the order of the stores are those of the plain loop.
#define QOC_TRACE_BATCH 8
__device__ __forceinline__ void ens_trace_rows(double* __restrict__ tu, size_t tstride, const double* __restrict__ delta, int q,
                                               const double* __restrict__ tr, size_t estride, int E) {
    int e = 0;
    for (; e + QOC_TRACE_BATCH <= E; e += QOC_TRACE_BATCH) {
        double v[QOC_TRACE_BATCH];
#pragma unroll
        for (int i = 0; i < QOC_TRACE_BATCH; ++i) v[i] = delta[(size_t)(e + i) * q] + tr[(size_t)(e + i) * estride];
#pragma unroll
        for (int i = 0; i < QOC_TRACE_BATCH; ++i) tu[(size_t)(e + i) * tstride] = v[i];
    }
    for (; e < E; ++e) tu[(size_t)e * tstride] = delta[(size_t)e * q] + tr[(size_t)e * estride];
}

// Trajectory controls from the group's: thread per (group, row j < k', slice), a loop over the members.  from_base: the group's controls
// are formed here from its variable (w = sin(base), u = maxA w: k_controls' arithmetic) and stored to the group view too; else they are the
// group's u (what the Adam tail left in u2 and the engine swapped in).  Also mirrors the group's done flag into its trajectories: the heavy
// kernels skip finished trajectories by their own flag.
// TRACES (k_ens_expand_traces, launched while a table is set): a frozen row is delta[e][q'] + tr[e][q'][t], one fp64 add where the row is
// written.  The slice is the thread's fastest index, so the members' reads are q steps apart and coalesced along t.  Without a table the
// engine launches k_ens_expand, whose code is what it was before the table existed.
template <bool TRACES>
__device__ __forceinline__ void ens_expand_body(const QocDev& t, const QocDev& g, const QocEns& en, int from_base) {
    const int steps = g.steps, k = g.k, kp = t.k, E = en.E;
    const size_t total = (size_t)g.B * kp * steps;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int tt = (int)(i % steps);
        const int j = (int)((i / steps) % kp);
        const int gi = (int)(i / ((size_t)steps * kp));
        double* tu = t.u + ((size_t)gi * E * kp + j) * steps + tt;
        const size_t tstride = (size_t)kp * steps;
        const size_t dev = (size_t)(gi / en.R) * E;                  // the first member row of this control set's device
        if (j < k) {
            const double* a = en.a + dev * k;
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
            for (int e = 0; e < E; ++e) t.done[(size_t)gi * E + e] = g.done[gi];
    }
}
__global__ void __launch_bounds__(256) k_ens_expand(QocDev t, QocDev g, QocEns en, int from_base) { ens_expand_body<false>(t, g, en, from_base); }
__global__ void __launch_bounds__(256) k_ens_expand_traces(QocDev t, QocDev g, QocEns en, int from_base) { ens_expand_body<true>(t, g, en, from_base); }

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
        const double* a = en.a + (size_t)(gi / en.R) * E * k;
        double acc = (en.wt[0] * a[j]) * src[o];
        for (int e = 1; e < E; ++e) acc = acc + (en.wt[e] * a[(size_t)e * k + j]) * src[(size_t)e * tstride + o];
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

// ---- risk-sensitive ensembles (qoc_set_risk, beta > 0): the soft worst case J = c_max + log1p(sum_e w_e expm1(beta (c_e - c_max))) / beta of
// the members' costs c_e = loss_e + reg_state_e in place of their weighted mean.  k_ens_tilt forms J and the tilted weights pi_e = dJ/dc_e of
// one control set; the _risk reduce kernels are k_ens_reduce / k_shape_reduce with pi + g E where those read en.wt, and leave the scalars alone.

#define QOC_TILT_BLOCK 256

// One workgroup per control set, launched after the backward kernels and before the reduce.  The transcendental work (expm1, exp: one each
// per member) is spread over the threads, members e = tid, tid + 256, ..; the maximum is exact in any order (threads, then an LDS tree); the
// two sums -- S over w_e expm1(x_e), reg_state over pi_e reg_state_e -- are added by thread 0 alone in the order 0 .. E-1 from member 0's
// term, out of the terms the threads left in pi[] (S) and of pi[] itself (reg_state): a few thousand dependent adds at most, beside G E
// trajectories of backward sweeps.  The maximum runs over the members with w_e > 0 (all of them, unless the caller gave a zero weight: such
// a member has pi_e = 0 and must not set the shift either).  No atomics, no contraction: two evaluations agree bit for bit.  A finished
// control set of a loop iteration keeps its values and weights.
__global__ void __launch_bounds__(QOC_TILT_BLOCK) k_ens_tilt(QocDev t, QocDev g, QocEns en, double beta, double* __restrict__ pi_all) {
#pragma clang fp contract(off)
    const int gi = blockIdx.x;
    if (g.skip_done && g.done[gi]) return;
    const int E = en.E, tid = threadIdx.x;
    const double* loss = t.loss + (size_t)gi * E;
    const double* reg = t.reg_state + (size_t)gi * E;
    double* pi = pi_all + (size_t)gi * E;
    __shared__ double red[QOC_TILT_BLOCK];
    __shared__ double bc;
    double m = -INFINITY;
    for (int e = tid; e < E; e += QOC_TILT_BLOCK) {
        const double c = loss[e] + reg[e];
        if (en.wt[e] > 0.0 && c > m) m = c;                  // (a NaN cost is no maximum, but reaches J through its x_e)
    }
    red[tid] = m;
    __syncthreads();
    for (int off = QOC_TILT_BLOCK / 2; off > 0; off >>= 1) {
        if (tid < off) { const double a = red[tid], b = red[tid + off]; red[tid] = b > a ? b : a; }
        __syncthreads();
    }
    const double cmax = red[0];
    for (int e = tid; e < E; e += QOC_TILT_BLOCK) {
        const double w = en.wt[e];
        pi[e] = w > 0.0 ? w * expm1(beta * ((loss[e] + reg[e]) - cmax)) : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        double S = pi[0];
        for (int e = 1; e < E; ++e) S = S + pi[e];
        bc = S;
    }
    __syncthreads();
    const double S = bc, den = 1.0 + S;
    for (int e = tid; e < E; e += QOC_TILT_BLOCK) {
        const double w = en.wt[e];
        pi[e] = w > 0.0 ? w * exp(beta * ((loss[e] + reg[e]) - cmax)) / den : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        double r = pi[0] * reg[0];
        for (int e = 1; e < E; ++e) r = r + pi[e] * reg[e];
        const double J = cmax + log1p(S) / beta;
        g.loss[gi] = J - r;
        g.reg_state[gi] = r;
    }
}

// k_ens_reduce with the control set's tilted weights: same grid, same member order from member 0's term; the scalars are k_ens_tilt's.
__global__ void __launch_bounds__(256) k_ens_reduce_risk(QocDev t, QocDev g, QocEns en, const double* __restrict__ pi_all) {
#pragma clang fp contract(off)
    const int gi = blockIdx.y;
    if (g.skip_done && g.done[gi]) return;
    const int steps = g.steps, k = g.k, kp = t.k, E = en.E, ks = k * steps;
    const size_t tstride = (size_t)kp * steps;
    const double* src = t.dLdu + (size_t)gi * E * tstride;
    const double* pi = pi_all + (size_t)gi * E;
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o < ks) {
        const int j = o / steps;
        const double* a = en.a + (size_t)(gi / en.R) * E * k;
        double acc = (pi[0] * a[j]) * src[o];
        for (int e = 1; e < E; ++e) acc = acc + (pi[e] * a[(size_t)e * k + j]) * src[(size_t)e * tstride + o];
        g.dLdu[(size_t)gi * ks + o] = acc;
    }
}
