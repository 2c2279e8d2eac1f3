// qoc_kernels_generic.h -- any-n complex-fp64 kernels (workgroup-cooperative products straight from HBM/L2).
// This is the correctness-first path for every (n, m, mode); the register-resident MFMA path
// (qoc_kernels_mfma.h) replaces the propagator kernels when n <= 32 in unitary mode.
//
// Reference call sites are cited as file:line relative to /root/reference/quantum_optimal_control/.
#pragma once
#include "qoc_common.h"
#include "qoc_state_source.h"

// C[MxN] = op(A)[MxKd] * B[KdxN]; row-major operands in global memory; all threads of the workgroup cooperate.
// No barrier inside: the caller synchronises before C is read.
template <bool CONJ_T_A>
__device__ __forceinline__ void wg_mm(int M, int N, int Kd, const cplx* __restrict__ A, int lda,
                                      const cplx* __restrict__ Bm, int ldb, cplx* __restrict__ C, int ldc) {
    for (int o = threadIdx.x; o < M * N; o += blockDim.x) {
        const int i = o / N, j = o - i * N;
        cplx acc = cmake(0.0, 0.0);
        for (int c = 0; c < Kd; ++c) {
            const cplx a = CONJ_T_A ? cconj(A[(size_t)c * lda + i]) : A[(size_t)i * lda + c];
            cfma(acc, a, Bm[(size_t)c * ldb + j]);
        }
        C[(size_t)i * ldc + j] = acc;
    }
}

// w = sin(base), u = maxA*w                                   core/tensorflow_state.py:176-178
__global__ void k_controls(QocDev d) {
    const int total = d.B * d.k * d.steps;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int kk = (i / d.steps) % d.k;
        const double w = sin(d.base[i]);
        d.w[i] = w;
        d.u[i] = d.maxA[kk] * w;
    }
}

// H_t = sum_ii (uks[ii]/2^s) * H_all[ii]                       tensorflow_state.py:30-33 (scaled) / :83-86 (s = 0)
__device__ __forceinline__ void wg_assemble(const QocDev& d, int b, int t, double inv_scale, double sign,
                                            cplx* __restrict__ A) {
    const int nn = d.n * d.n;
    const double* ub = d.u + (size_t)b * d.k * d.steps + t;
    for (int o = threadIdx.x; o < nn; o += blockDim.x) {
        cplx acc = cscale(d.Hs[o], sign * inv_scale);
        for (int kk = 0; kk < d.k; ++kk) {
            const double c = sign * (ub[(size_t)kk * d.steps] * inv_scale);
            const cplx h = d.Hs[(size_t)(kk + 1) * nn + o];
            acc.x = fma(c, h.x, acc.x);
            acc.y = fma(c, h.y, acc.y);
        }
        A[o] = acc;
    }
}

// K_t = (sum_{j<=T} A^j/j!)^(2^s)   -- matexp_op                tensorflow_state.py:25-46, 70-75
// Formed as K_t = I + E: E = sum_{1<=j<=T} A^j/j!, each squaring (I + E)^2 = I + (2E + E E), the identity added once at the end.  Squaring
// I + E itself rounds relative to the 1 on the diagonal and every squaring doubles that error: 2^s eps per slice, 1e-12 in unitary_scale
// over 50 slices at s = 12.  E stays of the size of the generator, so its rounding is relative to that and K_t is good to a few eps at every s.
// grid-stride over (seed, t); scratch: 3 n x n matrices per workgroup.
__global__ void __launch_bounds__(QOC_BLOCK) k_expm_generic(QocDev d, cplx* __restrict__ Kout, cplx* __restrict__ scratch) {
    const int nn = d.n * d.n;
    cplx* A = scratch + (size_t)blockIdx.x * 3 * nn;
    cplx* P = A + nn;
    cplx* Q = P + nn;
    const double inv_scale = 1.0 / (double)(1 << d.s);
    for (int item = blockIdx.x; item < d.B * d.steps; item += gridDim.x) {
        const int b = item / d.steps, t = item - b * d.steps;
        cplx* Kt = Kout + (size_t)item * nn;
        wg_assemble(d, b, t, inv_scale, 1.0, A);
        __syncthreads();
        for (int o = threadIdx.x; o < nn; o += blockDim.x) {       // ii = 1: matexp - I = H/1 ; H_n = H
            const cplx a = A[o];
            P[o] = a;
            Kt[o] = a;
        }
        __syncthreads();
        double fact = 1.0;
        for (int ii = 2; ii <= d.T; ++ii) {
            wg_mm<false>(d.n, d.n, d.n, A, d.n, P, d.n, Q, d.n);     // H_n = H * H_n            :41
            __syncthreads();
            fact *= (double)ii;
            for (int o = threadIdx.x; o < nn; o += blockDim.x) {    // matexp += H_n / factorial :40
                const cplx q = Q[o];
                cplx kv = Kt[o];
                kv.x += q.x / fact; kv.y += q.y / fact;
                Kt[o] = kv;
            }
            cplx* tmp = P; P = Q; Q = tmp;
            __syncthreads();
        }
        for (int sq = 0; sq < d.s; ++sq) {                          // squaring: E <- 2E + E E   :43-44
            wg_mm<false>(d.n, d.n, d.n, Kt, d.n, Kt, d.n, Q, d.n);
            __syncthreads();
            for (int o = threadIdx.x; o < nn; o += blockDim.x) {
                const cplx e = Kt[o], q = Q[o];
                Kt[o] = cmake((e.x + e.x) + q.x, (e.y + e.y) + q.y);
            }
            __syncthreads();
        }
        for (int i = threadIdx.x; i < d.n; i += blockDim.x) Kt[(size_t)i * d.n + i].x += 1.0;
    }
}

// Forward chain, one workgroup per seed:  X_t = K_t X_{t-1},  Psi_t = K_t Psi_{t-1} (= X_t V)
// tensorflow_state.py:204-227 (propagator), :229-242 (inter vectors). scratch: 2 n x n per seed.
__global__ void __launch_bounds__(QOC_BLOCK) k_fwd_generic(QocDev d, const cplx* __restrict__ Kin, cplx* __restrict__ scratch) {
    __shared__ double red[8];
    const int b = blockIdx.x, n = d.n, m = d.m, nn = n * n, nm = n * m;
    cplx* Xa = scratch + (size_t)b * 2 * nn;
    cplx* Xb = Xa + nn;
    cplx* iv = d.inter + (size_t)b * (d.steps + 1) * nm;
    for (int o = threadIdx.x; o < nn; o += blockDim.x) Xa[o] = d.U0[o];
    for (int o = threadIdx.x; o < nm; o += blockDim.x) iv[o] = d.V[o];
    __syncthreads();
    const cplx* psi_prev = d.Psi0;
    for (int t = 0; t < d.steps; ++t) {
        const cplx* Kt = Kin + ((size_t)b * d.steps + t) * nn;
        cplx* psi = iv + (size_t)(t + 1) * nm;
        wg_mm<false>(n, m, n, Kt, n, psi_prev, m, psi, m);
        wg_mm<false>(n, n, n, Kt, n, Xa, n, Xb, n);
        __syncthreads();
        cplx* tmp = Xa; Xa = Xb; Xb = tmp;
        psi_prev = psi;
    }
    // final_state and unitary_scale = (1/n) sum_ab Re (X^dagger X)_ab = (1/n) sum_c |sum_a X[c][a]|^2   :223-225
    double part = 0.0;
    for (int c = threadIdx.x; c < n; c += blockDim.x) {
        cplx rs = cmake(0.0, 0.0);
        for (int a = 0; a < n; ++a) rs = cadd(rs, Xa[c * n + a]);
        part += rs.x * rs.x + rs.y * rs.y;
    }
    for (int o = threadIdx.x; o < nn; o += blockDim.x) d.Xfinal[(size_t)b * nn + o] = Xa[o];
    const double tot = block_sum(part, red);
    if (threadIdx.x == 0) d.uscale[b] = tot / (double)n;
}

// State-transfer forward, one workgroup per seed: psi_{t+1} = sum_{j<T} B_t^j psi_t / j!  (matvecexp_op)
// tensorflow_state.py:77-97, 244-261.  scratch per seed: n*n (B_t) + 2*n*m.
__global__ void __launch_bounds__(QOC_BLOCK) k_st_fwd_generic(QocDev d, cplx* __restrict__ scratch) {
    const int b = blockIdx.x, n = d.n, m = d.m, nn = n * n, nm = n * m;
    cplx* Bt = scratch + (size_t)b * (nn + 2 * nm);
    cplx* pa = Bt + nn;
    cplx* pb = pa + nm;
    cplx* iv = d.inter + (size_t)b * (d.steps + 1) * nm;
    for (int o = threadIdx.x; o < nm; o += blockDim.x) iv[o] = d.V[o];
    __syncthreads();
    for (int t = 0; t < d.steps; ++t) {
        const cplx* psi = iv + (size_t)t * nm;
        cplx* out = iv + (size_t)(t + 1) * nm;
        wg_assemble(d, b, t, 1.0, 1.0, Bt);
        for (int o = threadIdx.x; o < nm; o += blockDim.x) { pa[o] = psi[o]; out[o] = psi[o]; }
        __syncthreads();
        double fact = 1.0;
        for (int ii = 1; ii < d.T; ++ii) {
            wg_mm<false>(n, m, n, Bt, n, pa, m, pb, m);              // psi_n = H psi_n           :94
            __syncthreads();
            fact *= (double)ii;
            for (int o = threadIdx.x; o < nm; o += blockDim.x) {    // matvecexp += psi_n/fact   :95
                cplx v = out[o];
                v.x += pb[o].x / fact; v.y += pb[o].y / fact;
                out[o] = v;
            }
            cplx* tmp = pa; pa = pb; pb = tmp;
            __syncthreads();
        }
    }
}

// Forbidden levels (regularization_functions.py:71-85).  Dressed (:74-80): phi = <dressed level f | Psi_tau[:, j]> is an n-term dot product per
// (seed, time point, level, vector).  One thread each, the operands of eight terms in flight at a time: inside k_loss (one workgroup per
// seed, a dependent load per term) the same sums cost 0.22 ms per iteration of ONE C2 trajectory; source_at recomputed them for every row.
// Fd = 2 a_f |phi|^2 phi feeds source_at, Fpop = a_f |phi|^4 / 2 is the entry's share of the regulariser, summed by k_loss.
__global__ void __launch_bounds__(256) k_dress_amplitudes(QocDev d) {
    const int n = d.n, m = d.m, per_t = d.n_forb * m;
    const size_t per_b = (size_t)(d.steps + 1) * per_t, total = (size_t)d.B * per_b;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(o / per_b);
        if (d.skip_done && d.done[b]) continue;
        const size_t bt = o / per_t;                                             // b * (steps + 1) + tau
        const int fj = (int)(o - bt * per_t), f = fj / m, j = fj - f * m, st = d.forb_state[f];
        const cplx* p = d.inter + bt * n * m + j;
        if (!d.forbid_dressed) {                                                 // bare level: the amplitude is an entry of Psi (source_at reads it there)
            const cplx phi = p[(size_t)st * m];
            const double pop = phi.x * phi.x + phi.y * phi.y;
            d.Fpop[o] = d.forb_a[f] * 0.5 * pop * pop;
            continue;
        }
        const cplx* v = d.Vs + st;
        cplx phi = cmake(0.0, 0.0);
        for (int c0 = 0; c0 < n; c0 += 8) {
            cplx vv[8], pp[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) { const int c = min(c0 + q, n - 1); vv[q] = v[(size_t)c * n]; pp[q] = p[(size_t)c * m]; }
#pragma unroll
            for (int q = 0; q < 8; ++q) if (c0 + q < n) cfma_conj(phi, vv[q], pp[q]);
        }
        const double pop = phi.x * phi.x + phi.y * phi.y;
        d.Fd[o] = cscale(phi, 2.0 * d.forb_a[f] * pop);
        d.Fpop[o] = d.forb_a[f] * 0.5 * pop * pop;
    }
}

// speed_up (regularization_functions.py:88-95): the overlap z_tau = <W, Psi_tau> of every time point, a wave per (seed, time point).
// Inside k_loss (one workgroup per seed walking the time points, two block reductions each) these cost 0.65 ms per iteration of one C2
// trajectory, 0.9 ms for 64 seeds.
__global__ void __launch_bounds__(256) k_time_overlaps(QocDev d) {
    const int lane = threadIdx.x & 63, nm = d.n * d.m;
    const size_t total = (size_t)d.B * (d.steps + 1);
    for (size_t it = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); it < total; it += (size_t)gridDim.x * 4) {
        const int b = (int)(it / (d.steps + 1));
        if (d.skip_done && d.done[b]) continue;
        const cplx* p = d.inter + it * nm;
        double tr = 0.0, ti = 0.0;
        for (int o = lane; o < nm; o += 64) {
            const cplx f = p[o], w = d.W[o];
            tr += f.x * w.x + f.y * w.y;        // f * conj(w)
            ti += f.y * w.x - f.x * w.y;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { tr += __shfl_xor(tr, off, 64); ti += __shfl_xor(ti, off, 64); }
        if (lane == 0) d.ztau[it] = cmake(tr, ti);
    }
}

// Fidelity, state-side regulariser values and everything the sources need; one workgroup per seed.
// tensorflow_state.py:282-340, regularization_functions.py:71-95.
__global__ void __launch_bounds__(QOC_BLOCK) k_loss(QocDev d) {
    __shared__ double red[8];
    const int b = blockIdx.x, n = d.n, m = d.m, nm = n * m;
    const cplx* iv = d.inter + (size_t)b * (d.steps + 1) * nm;
    const cplx* fin = iv + (size_t)d.steps * nm;
    double zr = 0.0, zi = 0.0, nrm = 0.0;
    for (int o = threadIdx.x; o < nm; o += blockDim.x) {
        const cplx f = fin[o], w = d.W[o];
        zr += f.x * w.x + f.y * w.y;        // f * conj(w)
        zi += f.y * w.x - f.x * w.y;
        nrm += f.x * f.x + f.y * f.y;
    }
    zr = block_sum(zr, red); zi = block_sum(zi, red); nrm = block_sum(nrm, red);
    const double mm = (double)m * (double)m;
    double reg_state = 0.0;
    if (d.has_speed) {                                                           // :88-95  (z_tau: k_time_overlaps)
        double val = 0.0;
        for (int tau = threadIdx.x; tau <= d.steps; tau += blockDim.x) {
            const cplx z = d.ztau[(size_t)b * (d.steps + 1) + tau];
            val += (z.x * z.x + z.y * z.y) / mm;
        }
        val = block_sum(val, red);
        const double resid = (double)(d.steps + 1) - val;
        if (threadIdx.x == 0) d.su_resid[b] = resid;
        reg_state += d.a_speed * 0.5 * resid * resid;
    }
    if (d.n_forb > 0) {                                                          // :71-85
        double acc = 0.0;
        const int total = (d.steps + 1) * m;
        for (int o = threadIdx.x; o < total; o += blockDim.x) {                  // a_f |phi|^4 / 2 of every (time point, level, vector): k_dress_amplitudes
            const int tau = o / m, j = o - tau * m;
            for (int f = 0; f < d.n_forb; ++f) acc += d.Fpop[(((size_t)b * (d.steps + 1) + tau) * d.n_forb + f) * m + j];
        }
        reg_state += block_sum(acc, red);
    }
    if (threadIdx.x == 0) {
        d.zfin[b] = cmake(zr, zi);
        d.loss[b] = 1.0 - (zr * zr + zi * zi) / mm;
        d.reg_state[b] = reg_state;
        if (d.state_transfer) d.uscale[b] = nrm * nrm / mm;                      // tensorflow_state.py:335
    }
    if (d.uscale_in_loss && !d.state_transfer) {              // unitary_scale = (1/n) sum_c |sum_a X[c][a]|^2   tensorflow_state.py:225
        const cplx* X = d.Xfinal + (size_t)b * n * n;
        double part = 0.0;
        for (int c = threadIdx.x; c < n; c += blockDim.x) {
            cplx rs = cmake(0.0, 0.0);
            for (int a = 0; a < n; ++a) rs = cadd(rs, X[c * n + a]);
            part += rs.x * rs.x + rs.y * rs.y;
        }
        part = block_sum(part, red);
        if (threadIdx.x == 0) d.uscale[b] = part / (double)n;
    }
}


// dL/du_{k,t} = Re <Lambda_t, H_k' Psi_t>                      tensorflow_state.py:61-63 / :112-114
__device__ __forceinline__ void wg_control_grads(const QocDev& d, int b, int t, const cplx* __restrict__ lam,
                                                 const cplx* __restrict__ psi, double* red) {
    const int n = d.n, m = d.m, nm = n * m, nn = n * n;
    for (int kk = 0; kk < d.k; ++kk) {
        const cplx* Hk = d.Hs + (size_t)(kk + 1) * nn;
        double part = 0.0;
        for (int o = threadIdx.x; o < nm; o += blockDim.x) {
            const int i = o / m, j = o - i * m;
            cplx y = cmake(0.0, 0.0);
            for (int c = 0; c < n; ++c) cfma(y, Hk[i * n + c], psi[c * m + j]);
            part += lam[o].x * y.x + lam[o].y * y.y;                  // Re(conj(lam) * y)
        }
        const double g = block_sum(part, red);
        if (threadIdx.x == 0) d.dLdu[((size_t)b * d.k + kk) * d.steps + t] = g;
    }
}

__device__ __forceinline__ void wg_terminal_costate(const QocDev& d, int b, bool need_src, cplx* __restrict__ lam) {
    const int nm = d.n * d.m;
    const cplx z = d.zfin[b];
    const double c0 = -2.0 / ((double)d.m * (double)d.m);
    for (int o = threadIdx.x; o < nm; o += blockDim.x) {
        cplx v = cscale(cmul(z, d.W[o]), c0);
        if (need_src) v = cadd(v, source_at(d, b, d.steps, o / d.m, o % d.m));
        lam[o] = v;
    }
}

// Backward sweep (unitary mode), one workgroup per seed: Lambda_{t-1} = K_t^dagger Lambda_t + S_{t-1}.
__global__ void __launch_bounds__(QOC_BLOCK) k_bwd_generic(QocDev d, const cplx* __restrict__ Kin, cplx* __restrict__ scratch) {
    __shared__ double red[8];
    const int b = blockIdx.x, n = d.n, m = d.m, nn = n * n, nm = n * m;
    cplx* la = scratch + (size_t)b * 2 * nm;
    cplx* lb = la + nm;
    const cplx* iv = d.inter + (size_t)b * (d.steps + 1) * nm;
    const bool need_src = d.n_forb > 0 || d.has_speed;
    wg_terminal_costate(d, b, need_src, la);
    __syncthreads();
    for (int t = d.steps - 1; t >= 0; --t) {
        wg_control_grads(d, b, t, la, iv + (size_t)(t + 1) * nm, red);
        if (t == 0) break;
        const cplx* Kt = Kin + ((size_t)b * d.steps + t) * nn;
        wg_mm<true>(n, m, n, Kt, n, la, m, lb, m);
        __syncthreads();
        if (need_src) {
            for (int o = threadIdx.x; o < nm; o += blockDim.x) lb[o] = cadd(lb[o], source_at(d, b, t, o / m, o % m));
        }
        cplx* tmp = la; la = lb; lb = tmp;
        __syncthreads();
    }
}

// Backward sweep (state transfer): lambda_t = sum_{j<T} (-B_t)^j lambda_{t+1} / j! + S_t   tensorflow_state.py:100-133
__global__ void __launch_bounds__(QOC_BLOCK) k_st_bwd_generic(QocDev d, cplx* __restrict__ scratch) {
    __shared__ double red[8];
    const int b = blockIdx.x, n = d.n, m = d.m, nn = n * n, nm = n * m;
    cplx* Bt = scratch + (size_t)b * (nn + 3 * nm);
    cplx* lam = Bt + nn;
    cplx* pa = lam + nm;
    cplx* pb = pa + nm;
    const cplx* iv = d.inter + (size_t)b * (d.steps + 1) * nm;
    const bool need_src = d.n_forb > 0 || d.has_speed;
    wg_terminal_costate(d, b, need_src, lam);
    __syncthreads();
    for (int t = d.steps - 1; t >= 0; --t) {
        wg_control_grads(d, b, t, lam, iv + (size_t)(t + 1) * nm, red);
        if (t == 0) break;
        wg_assemble(d, b, t, 1.0, -1.0, Bt);                         // H = sum (-uks) H_all      :121-123
        for (int o = threadIdx.x; o < nm; o += blockDim.x) pa[o] = lam[o];
        __syncthreads();
        double fact = 1.0;
        for (int ii = 1; ii < d.T; ++ii) {
            wg_mm<false>(n, m, n, Bt, n, pa, m, pb, m);
            __syncthreads();
            fact *= (double)ii;
            for (int o = threadIdx.x; o < nm; o += blockDim.x) {
                cplx v = lam[o];
                v.x += pb[o].x / fact; v.y += pb[o].y / fact;
                lam[o] = v;
            }
            cplx* tmp = pa; pa = pb; pb = tmp;
            __syncthreads();
        }
        if (need_src) {
            for (int o = threadIdx.x; o < nm; o += blockDim.x) lam[o] = cadd(lam[o], source_at(d, b, t, o / m, o % m));
            __syncthreads();
        }
    }
}
