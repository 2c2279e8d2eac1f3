// qoc_engine.hip -- host side of libqoc_hip.so: the C ABI of include/qoc.h over the HIP kernels.
//
// One engine handle == one GRAPE problem (shared Hamiltonians, n_seeds independent control sets) resident in the
// HBM of one MI355X, one HIP stream.  One iteration is a fixed sequence of kernel launches on that stream; the
// stop rule, learning-rate schedule and Adam update run on the device, so the host never has to synchronise
// inside the optimisation loop (it only polls the done flags every `poll_every` iterations).
#include "../../include/qoc.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "qoc_common.h"
#include "qoc_kernels_finish.h"
#include "qoc_kernels_generic.h"
#include "qoc_kernels_mfma.h"
#include "qoc_kernels_st.h"
#include "qoc_kernels_gemm.h"
#include "qoc_gemm_ts.h"
#include "qoc_small.h"
#include "qoc_ensemble.h"
#include "qoc_transfer.h"
#include "qoc_control_map.h"
#include "qoc_exact_grad.h"
#include "qoc_lindblad.h"
#include "qoc_lindblad_tiled.h"
#include "qoc_sparse.h"
#include "qoc_sparse_host.h"
#include "qoc_lbfgs.h"

#include "qoc_plan_limits.h"            // the measured numbers of AUTO's table (QOC_PLAN_*), shared with tests/test_auto_plan.py
// (QOC_PLAN_LAT_WORK = 4608 seeds x time slices: since the batch sweeps take their chunk boundaries and final_state from k_mfma_bnd_scan
// the batch kernels are ahead from 10 seeds of 500 slices on -- 0.356 ms at 12 seeds against 0.444; 8 seeds: 0.349 against 0.305;
// profiles/r03_latency_sweep.txt)
static thread_local std::string g_err;

static int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                                                               \
    do {                                                                                                                            \
        hipError_t e_ = (expr);                                                                                                     \
        if (e_ != hipSuccess) return fail(QOC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);  \
    } while (0)

#define HIP_TRY_MSG(expr, ...) do { if ((expr) != hipSuccess) return fail(QOC_ERR_HIP, __VA_ARGS__); } while (0)
#define TRY(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)

struct qoc_engine {
    qoc_config cfg;
    QocDev d;
    int path;
    int chunks;
    hipStream_t stream;
    std::vector<void*> allocs;
    char* arena_cur = nullptr;      // bump allocator over the chunks in `allocs` (dev_alloc)
    size_t arena_left = 0;
    // generic path
    cplx* K = nullptr;          // [B][steps][n][n]
    cplx* expm_scratch = nullptr;
    int expm_grid = 0;
    cplx* seed_scratch = nullptr;
    double* fin_part = nullptr;      // [B][fin_S + 2][2] partial sums of the split tail (k_finish_split_a / _b: control sets of 4097 .. 8192 (k, t) elements)
    int fin_S = 0;
    // mfma path
    QocMfma mf;
    QocMfmaPlan mp;            // its launches, resolved by qoc_mfma_setup
    QocGemm gm;
    QocSmall sm;                // workgroup-resident path (csrc/qoc_small.h)
    bool evaluated = false;
    // QOC_DEBUG_SKIP (timing experiments only): 1 controls, 2 exponentials, 4 forward, 8 loss, 16 backward, 32 finish
    int skip_mask = 0;
    // u2 / w2 hold maxA sin(base) of the CURRENT variable (written by the Adam tail or by qoc_get_uks)
    bool controls_ready = false;
    bool final_stale = false, inter_stale = false;   // MFMA latency mode: Xfinal / uscale not yet formed for the last evaluation
    double* step_lr = nullptr;  // [B] per-seed learning rates of qoc_adam_step
    // profiling of the dominant kernel
    bool profiling = false;
    std::vector<hipEvent_t> ev;  // pairs
    size_t ev_used = 0;
    double prof_ms = 0.0;
    int64_t prof_launches = 0;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    // robust ensemble (qoc_create_ensemble, csrc/qoc_ensemble.h): d is then the TRAJECTORY view (G E trajectories, k + q controls, read by
    // the heavy kernels) and g the GROUP view (G control sets, k controls: variable, Adam slots, stop rule, pulse regularisers, the tail)
    int ens_E = 0;
    int fleet_F = 0;                // qoc_create_fleet: devices, each with its own member table (en.R control sets per device); else 0
    QocDev g;
    QocEns en{};
    std::vector<double> ens_wt;     // host copy of the weights (unitary_scale of a group is formed on read-back)
    // risk-sensitive objective (qoc_set_risk, k_ens_tilt): beta > 0 replaces the weighted mean by the soft worst case over the members
    double risk_beta = 0.0;
    double* risk_pi = nullptr;      // [G][E] tilted weights of the last evaluation, allocated by the first qoc_set_risk with beta > 0
    // noise traces (qoc_set_traces): [F][E][q][steps] added to the frozen rows per slice; en.tr points at it while a table is set
    double* traces = nullptr;       // allocated by the first qoc_set_traces with a table, kept (and overwritten) afterwards
    // transfer-function GRAPE (qoc_create_shaped, csrc/qoc_transfer.h): an ensemble engine whose group view is the SAMPLE view (P samples per
    // control in place of the time slices) and whose glue kernels apply the response matrix
    bool shaped = false;
    QocShape sh{};
    // control map (qoc_create_mapped, csrc/qoc_control_map.h): an ensemble engine whose member glue works on the PULSE view pv (k + q rows, staging
    // arrays for u / dLdu, the trajectories' own loss / reg_state / done); k_map_expand / k_map_reduce join it and the trajectory view (r + q rows)
    bool mapped = false;
    QocMap cm{};
    QocDev pv;
    // exact gradient (qoc_config.gradient = 1, csrc/qoc_exact_grad.h): the generic path's forward, a costate-storing sweep and k_exact_grad
    QocExact xg{};
    // open-system GRAPE (qoc_create_open, csrc/qoc_lindblad.h): density operators of the pairs of states of interest under a Lindblad master equation
    QocLb lb{};
    // the same past the LDS rule (QOC_PATH_LINDBLAD_TILED, csrc/qoc_lindblad_tiled.h): the operators in global scratch, the products on the matrix pipe
    QocLbt lbt{};
    // sparse state transfer (qoc_create_sparse, csrc/qoc_sparse.h): ELLPACK operators, no n x n array anywhere (d.Hs, d.U0 and d.Xfinal stay null)
    QocSparse sp{};
    std::vector<int> sp_widths;     // [k+1] W_j, for qoc_plan_describe
    bool sp_fleet_entry = false;    // made by qoc_create_sparse_fleet: qoc_plan_describe names the row layout
    // device-resident L-BFGS loop (qoc_iterate_lbfgs / qoc_run_lbfgs, csrc/qoc_lbfgs.h): per-set state, allocated by the first call for lq_cap pairs
    QocLbfgsDev lq{};
    int lq_cap = 0;
};

// the view that holds the control sets: the engine itself, or the group view of an ensemble engine
static inline QocDev& sets(qoc_engine* e) { return e->ens_E ? e->g : e->d; }
static inline const QocDev& sets(const qoc_engine* e) { return e->ens_E ? e->g : e->d; }
// a grid of one workgroup per `per_block` items, at most `cap` workgroups (the kernels stride over the rest)
static inline unsigned grid_for(size_t items, unsigned per_block, unsigned cap) {
    return (unsigned)std::min<size_t>((items + per_block - 1) / per_block, cap);
}

template <typename T>
static int dev_alloc(qoc_engine* e, T** p, size_t count) {
    // bump allocation out of 64 MB-granular chunks (qoc_arena_bytes: where many small recycled blocks land decides the speed)
    if (count == 0) count = 1;
    const size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
    if (bytes > e->arena_left) {
        void* q = nullptr;
        const size_t chunk = qoc_arena_bytes(bytes);
        hipError_t err = hipMalloc(&q, chunk);
        if (err != hipSuccess) return fail(QOC_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", chunk, hipGetErrorString(err));
        e->allocs.push_back(q);
        e->arena_cur = (char*)q;
        e->arena_left = chunk;
    }
    *p = (T*)e->arena_cur;
    e->arena_cur += bytes;
    e->arena_left -= bytes;
    return QOC_OK;
}

// ... cleared (`who`: the entry point that the message names)
template <typename T>
static int dev_zalloc(qoc_engine* e, T** p, size_t count, const char* who) {
    TRY(dev_alloc(e, p, count));
    HIP_TRY_MSG(hipMemset(*p, 0, count * sizeof(T)), "%s: clearing the state buffers failed", who);
    return QOC_OK;
}
template <typename T>
static int dev_upload(qoc_engine* e, const T** p, const T* host, size_t count) {
    T* q = nullptr;
    TRY(dev_alloc(e, &q, count));
    HIP_TRY(hipMemcpy(q, host, count * sizeof(T), hipMemcpyHostToDevice));
    *p = q;
    return QOC_OK;
}

static int prof_begin(qoc_engine* e) {
    if (!e->profiling) return QOC_OK;
    if (e->ev_used + 2 > e->ev.size()) {
        for (int i = 0; i < 2; ++i) {
            hipEvent_t x;
            HIP_TRY(hipEventCreate(&x));
            e->ev.push_back(x);
        }
    }
    HIP_TRY(hipEventRecord(e->ev[e->ev_used], e->stream));
    return QOC_OK;
}
static int prof_end(qoc_engine* e) {
    if (!e->profiling) return QOC_OK;
    HIP_TRY(hipEventRecord(e->ev[e->ev_used + 1], e->stream));
    e->ev_used += 2;
    return QOC_OK;
}
static int prof_collect(qoc_engine* e) {
    if (e->ev_used == 0) return QOC_OK;
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t i = 0; i < e->ev_used; i += 2) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e->ev[i], e->ev[i + 1]));
        e->prof_ms += ms;
        e->prof_launches += 1;
    }
    e->ev_used = 0;
    return QOC_OK;
}

// ---- one evaluation (+ optional on-device stop rule / Adam), enqueued on the engine stream ------------------------
// band_tw[r] = e^{-2 pi i r / N}, r < N: the direct DFT of the bandpass regulariser evaluated sincos for every (frequency, slice) pair --
// 2 k N^2 of them per seed and iteration, 1.7 ms for one C2 trajectory; the phase index f t mod N advances by additions instead
__global__ void __launch_bounds__(256) k_band_twiddles(cplx* tw, int N) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < N) { double c, s; unit_phase(r, 1, N, &c, &s); tw[r] = cmake(c, s); }
}

// Bandpass regulariser (regularization_functions.py:47-67) by direct DFT, outside the one-workgroup-per-seed finish kernel (where the
// 2 k N^2 terms of a seed took 0.4 ms of one C2 trajectory even with the phase table):
// k_band_spectrum: a wave per (seed, control, frequency): F_f = sum_t w_t e^{-2 pi i f t/N}; band_mag = cnt_f |F_f|, band_ph = cnt_f
// conj(F_f)/|F_f|
//   k_band_gradient: a thread per (seed, control, slice): band_dR = sum_f Re(band_ph_f e^{-2 pi i f t/N})
// cnt_f = how often the reference's two slices (f < lo; hi <= f < N/2) contain f.
__global__ void __launch_bounds__(256) k_band_spectrum(QocDev d) {
    const int steps = d.steps, lane = threadIdx.x & 63, half = steps / 2;
    const int lo = min(max(d.band_lo, 0), steps), hi = min(max(d.band_hi, 0), steps);
    const size_t total = (size_t)d.B * d.k * steps;
    for (size_t o = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); o < total; o += (size_t)gridDim.x * 4) {
        const int f = (int)(o % steps);
        const size_t bk = o / steps;
        if (d.skip_done && d.done[bk / d.k]) continue;
        const int cnt = (f < lo ? 1 : 0) + ((f >= hi && f < half) ? 1 : 0);
        cplx p = cmake(0.0, 0.0);
        double mg = 0.0;
        if (cnt > 0) {                                                       // (uniform over the wave)
            const double* wk = d.w + bk * steps;
            int r = (int)(((long long)f * lane) % steps);
            const int dr = (int)(((long long)f * 64) % steps);
            double fr = 0.0, fi = 0.0;
            for (int t = lane; t < steps; t += 64) {
                const cplx e = d.band_tw[r];
                fr = fma(wk[t], e.x, fr);
                fi = fma(wk[t], e.y, fi);
                r += dr; if (r >= steps) r -= steps;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { fr += __shfl_xor(fr, off, 64); fi += __shfl_xor(fi, off, 64); }
            const double mag = sqrt(fr * fr + fi * fi);
            mg = (double)cnt * mag;
            if (mag > 0.0) p = cmake((double)cnt * fr / mag, -(double)cnt * fi / mag);
        }
        if (lane == 0) { d.band_ph[o] = p; d.band_mag[o] = mg; }
    }
}
__global__ void __launch_bounds__(256) k_band_gradient(QocDev d) {
    const int steps = d.steps, half = steps / 2;
    const int lo = min(max(d.band_lo, 0), steps);
    const int fend = min(max(half, lo), steps);
    const size_t total = (size_t)d.B * d.k * steps;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const int t = (int)(o % steps);
        const size_t bk = o / steps;
        if (d.skip_done && d.done[bk / d.k]) continue;
        const cplx* pk = d.band_ph + bk * steps;
        double acc = 0.0;
        int r = 0;                                                           // f t mod steps, advanced by t per frequency
        for (int f0 = 0; f0 < fend; f0 += 8) {
            cplx qv[8], e[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                qv[q] = pk[min(f0 + q, fend - 1)];
                e[q] = d.band_tw[r];
                r += t; if (r >= steps) r -= steps;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q)
                // Re(ph_f e^{-2 pi i f t/N}); ph = 0 outside the counted bins
                if (f0 + q < fend) acc += qv[q].x * e[q].x - qv[q].y * e[q].y;
        }
        d.band_dR[o] = acc;
    }
}

// k_loss, preceded by what it needs per time point: the dressed-basis amplitudes of the forbidden levels, the overlaps of speed_up
static inline void launch_loss(const QocDev& d, hipStream_t s) {
    if (d.n_forb > 0)
        hipLaunchKernelGGL(k_dress_amplitudes, dim3(grid_for((size_t)d.B * (d.steps + 1) * d.n_forb * d.m, 256, 4096)), dim3(256), 0, s, d);
    if (d.has_speed) hipLaunchKernelGGL(k_time_overlaps, dim3(grid_for((size_t)d.B * (d.steps + 1), 4, 4096)), dim3(256), 0, s, d);
    hipLaunchKernelGGL(k_loss, dim3(d.B), dim3(QOC_BLOCK), 0, s, d);
}
// u / w = maxA sin(base) of every control set of the view
static inline void launch_controls(const QocDev& v, hipStream_t s) {
    hipLaunchKernelGGL(k_controls, dim3(grid_for((size_t)v.B * v.k * v.steps, QOC_BLOCK, 2048)), dim3(QOC_BLOCK), 0, s, v);
}

// workgroup-resident path: ONE launch runs `iters` loop iterations (or one evaluation / explicit step)
static int enqueue_small(qoc_engine* e, const QocAdamDev& ap, int iters) {
    QocDev d = e->d;
    d.skip_done = ap.mode == 1 ? 1 : 0;
    std::string msg;
    TRY(prof_begin(e));
    const int rc = qoc_small_launch(e->sm, d, ap, iters, e->stream, msg);
    if (rc) return fail(rc == -1 ? QOC_ERR_INVALID : QOC_ERR_HIP, "workgroup-resident iteration: %s", msg.c_str());
    TRY(prof_end(e));
    HIP_TRY(hipGetLastError());
    e->evaluated = true;
    e->controls_ready = false;                 // the kernel forms its own controls from the variable; d.u / d.w hold those of the last evaluation
    e->final_stale = true;                     // final_state, unitary_scale and inter_vecs are formed on read-back (refresh_small)
    e->inter_stale = true;
    return QOC_OK;
}

// Which kernel runs the tail of an iteration (regularisers, chain rule, stop rule, Adam; qoc_kernels_finish.h): a function of the engine alone,
// used by enqueue_iteration to launch it (and to tell qoc_gemm_backward who sums its gradient partials) and by qoc_plan_describe to report it
enum TailKind {
    TAIL_IN_LAUNCH,          // workgroup-resident path: inside its own launch
    TAIL_LATENCY_FUSED,      // MFMA latency mode without bandpass: the last-arriving workgroup of a seed in k_mfma_grad_lat* (64 (16 / NT) NT threads)
    TAIL_SPLIT,              // k_finish_split_a / _b over fin_S workgroups per control set
    TAIL_SPLIT_PARTIALS,     // ... part A summing the per-tile gradient partials of the GEMM path's persistent chains (no k_gemm_grad_reduce_wide)
    TAIL_FINISH4,            // k_finish_t<., 4>: 256 threads below 2048 elements per control set, else 1024
    TAIL_FINISH8,            // k_finish_t<., 8>: 4097 .. 8192 elements without the split tail (QOC_EXPERIMENTAL=1 QOC_FINISH_SPLIT=0)
};

static TailKind tail_kind(const qoc_engine* e) {
    const QocDev& d = sets(e);
    const int ks = d.k * d.steps;
    // an ensemble runs the stand-alone tails on its group view: never on one of the paths with a tail of their own, and its gradient is a
    // plain array (k_ens_reduce), never the persistent chains' partials
    if (e->ens_E) return ks > 4 * 1024 && e->fin_part ? TAIL_SPLIT : (ks <= 8 * 1024 && ks > 4 * 1024 ? TAIL_FINISH8 : TAIL_FINISH4);
    if (e->path == QOC_PATH_SMALL) return TAIL_IN_LAUNCH;
    if (e->path == QOC_PATH_MFMA && e->mp.tail_fusable && !d.has_band && !(e->skip_mask & (16 | 32)))
        return TAIL_LATENCY_FUSED;
    if (ks > 4 * 1024 && e->fin_part)
        return e->path == QOC_PATH_GEMM && qoc_gemm_chain_routes(e->gm) && e->skip_mask == 0 ? TAIL_SPLIT_PARTIALS : TAIL_SPLIT;
    return ks <= 8 * 1024 && ks > 4 * 1024 ? TAIL_FINISH8 : TAIL_FINISH4;
}

// ---- the four stages of enqueue_iteration, in launch order, on this iteration's copies d (trajectories) and gd (groups of an ensemble)
// 1. controls.  All read u / w: from k_controls, or -- swap_in: the Adam tail of the previous iteration (or qoc_get_uks) left them in
// u2 / w2 -- from no launch at all: enqueue_iteration has swapped the two pairs (in the engine's own views, so before it took the copies d
// and gd that the stages share).  own_controls: the slice kernel of the n <= 32 latency mode forms its own
static void enqueue_controls(const qoc_engine* e, const QocDev& d, const QocDev& gd, bool own_controls, bool swap_in) {
    const dim3 eg(grid_for((size_t)gd.B * d.k * d.steps, QOC_BLOCK, 2048));        // (ensembles: a thread per member's control)
    if (e->skip_mask & 1) return;
    if (!e->ens_E) {
        if (!own_controls && !swap_in) launch_controls(d, e->stream);
    } else if (!e->shaped) {
        // every member's controls from its group's (formed from the variable unless the last tail left them), and the done flags
        // (a trace table: the instance that adds it to the frozen rows; without one, the kernel of every engine so far)
        if (e->en.tr) hipLaunchKernelGGL(k_ens_expand_traces, eg, dim3(QOC_BLOCK), 0, e->stream, d, gd, e->en, swap_in ? 0 : 1);
        else hipLaunchKernelGGL(k_ens_expand, eg, dim3(QOC_BLOCK), 0, e->stream, d, gd, e->en, swap_in ? 0 : 1);
    } else {
        // a pulse response: the samples w_s / u_s from the variable (unless the last tail left them), then the pulse through the response
        if (!swap_in) launch_controls(gd, e->stream);
        if (e->en.tr) hipLaunchKernelGGL(k_shape_expand_traces, eg, dim3(QOC_BLOCK), 0, e->stream, d, gd, e->en, e->sh);
        else hipLaunchKernelGGL(k_shape_expand, eg, dim3(QOC_BLOCK), 0, e->stream, d, gd, e->en, e->sh);
    }
}
// 2. trajectories: exponentials, forward, loss, backward of the engine's path; qoc_profile_read's hipEvent bracket around the dominant one
static int enqueue_trajectories(qoc_engine* e, const QocDev& d, const QocAdamDev& ap, TailKind tail) {
    const int skip = e->skip_mask;
    const bool fused_tail = tail == TAIL_LATENCY_FUSED;
    if (e->path == QOC_PATH_MFMA) {
        TRY(prof_begin(e));
        if (!(skip & 2)) qoc_mfma_launch_expm(e->mp, e->mf, d, e->stream);
        TRY(prof_end(e));
        if (!(skip & 4)) qoc_mfma_launch_forward(e->mp, e->mf, d, e->stream);
        if (skip & 64) qoc_mfma_launch_forward(e->mp, e->mf, d, e->stream);        // debug: the same launch again (cold-start vs steady cost)
        if (skip & 128) qoc_mfma_launch_backward(e->mp, e->mf, d, e->stream);
        // latency mode / k_mfma_downup: inside the backward kernel
        if (!(skip & 8) && e->mp.engine_loss) launch_loss(d, e->stream);
        if (!(skip & 16)) {
            if (fused_tail) qoc_mfma_latency_gradient(e->mp, e->mf, d, &ap, e->stream);
            else qoc_mfma_launch_backward(e->mp, e->mf, d, e->stream);
        }
    } else if (e->path == QOC_PATH_GEMM && e->gm.ts_G > 0) {            // one trajectory sharded along the time axis (qoc_gemm_ts.h)
        const int rc = qoc_gemm_ts_evaluate(e->gm, d, e->stream, [&]() { launch_loss(d, e->stream); }, [&]() { return prof_begin(e); },
            [&]() { return prof_end(e); });
        if (rc == 1) return fail(QOC_ERR_HIP, "time-sharded iteration: clearing the gradient array failed");
        if (rc) return rc;                                              // (the message is the collective's / the profiler's)
    } else if (e->path == QOC_PATH_GEMM) {
        // the bracket: the exponentials -- or, on the direct state-transfer route (no exponentials: the assembly of the generators is all
        // qoc_gemm_expm does there), the backward half of the iteration, which the backward Taylor chain dominates
        const bool bracket_bwd = e->gm.route == QOC_GEMM_DIRECT;
        if (!bracket_bwd) TRY(prof_begin(e));
        qoc_gemm_expm(e->gm, d, e->stream);
        if (!bracket_bwd) TRY(prof_end(e));
        qoc_gemm_forward(e->gm, d, e->stream);
        launch_loss(d, e->stream);
        if (bracket_bwd) TRY(prof_begin(e));
        qoc_gemm_backward(e->gm, d, e->stream, tail == TAIL_SPLIT_PARTIALS);       // (the split tail sums the gradient partials: one launch less)
        if (bracket_bwd) TRY(prof_end(e));
    } else if (e->path == QOC_PATH_LINDBLAD) {                          // open system: forward, backward, reduce (csrc/qoc_lindblad.h)
        TRY(prof_begin(e));
        qoc_lb_forward(e->lb, d, e->stream);
        TRY(prof_end(e));
        qoc_lb_backward(e->lb, d, e->stream);
    } else if (e->path == QOC_PATH_LINDBLAD_TILED) {                    // the same on tiles in global scratch (csrc/qoc_lindblad_tiled.h)
        TRY(prof_begin(e));
        qoc_lbt_forward(e->lb, e->lbt, d, e->stream);
        TRY(prof_end(e));
        qoc_lbt_backward(e->lb, e->lbt, d, e->stream);
    } else if (e->path == QOC_PATH_SPARSE) {                            // sparse state transfer: forward, loss, costates + gradient (csrc/qoc_sparse.h)
        TRY(prof_begin(e));
        qoc_sp_forward(e->sp, d, e->stream);
        TRY(prof_end(e));
        launch_loss(d, e->stream);
        qoc_sp_backward(e->sp, d, e->stream);
    } else if (e->path == QOC_PATH_ST_FUSED) {
        TRY(prof_begin(e));
        st_fused_launch(d, e->stream, true);
        TRY(prof_end(e));
        launch_loss(d, e->stream);
        st_fused_launch(d, e->stream, false);
    } else {                                            // the any-size kernels; state transfer: no propagators, one sweep each way
        const bool st = d.state_transfer;
        TRY(prof_begin(e));
        if (st) hipLaunchKernelGGL(k_st_fwd_generic, dim3(d.B), dim3(QOC_BLOCK), 0, e->stream, d, e->seed_scratch);
        else hipLaunchKernelGGL(k_expm_generic, dim3(e->expm_grid), dim3(QOC_BLOCK), 0, e->stream, d, e->K, e->expm_scratch);
        TRY(prof_end(e));
        if (!st) hipLaunchKernelGGL(k_fwd_generic, dim3(d.B), dim3(QOC_BLOCK), 0, e->stream, d, e->K, e->seed_scratch);
        launch_loss(d, e->stream);
        if (e->xg.on) qoc_exact_backward(e->xg, d, st ? nullptr : e->K, st ? e->seed_scratch : nullptr, e->stream);
        else if (st) hipLaunchKernelGGL(k_st_bwd_generic, dim3(d.B), dim3(QOC_BLOCK), 0, e->stream, d, e->seed_scratch);
        else hipLaunchKernelGGL(k_bwd_generic, dim3(d.B), dim3(QOC_BLOCK), 0, e->stream, d, e->K, e->seed_scratch);
    }
    return QOC_OK;
}
// the soft worst case of one member is that member, whatever beta: a one-member ensemble keeps the mean's launches
static inline bool risk_on(const qoc_engine* e) { return e->risk_beta > 0.0 && e->ens_E > 1; }
// 3. an ensemble: the members' gradients and losses, weighted, into the group view
static void enqueue_ens_reduce(const qoc_engine* e, const QocDev& d, const QocDev& gd) {
    const int ks = gd.k * gd.steps;
    const dim3 per_thread((unsigned)((ks + 255) / 256), (unsigned)gd.B), per_wave((unsigned)((ks + 3) / 4), (unsigned)gd.B);
    if (risk_on(e)) {
        // the tilted weights and the scalars of every control set from its members' costs, then the same reduce with those weights
        hipLaunchKernelGGL(k_ens_tilt, dim3((unsigned)gd.B), dim3(QOC_TILT_BLOCK), 0, e->stream, d, gd, e->en, e->risk_beta, e->risk_pi);
        if (!e->shaped) hipLaunchKernelGGL(k_ens_reduce_risk, per_thread, dim3(256), 0, e->stream, d, gd, e->en, e->risk_pi);
        else if (e->sh.col_band <= QOC_SHAPE_WAVE_FROM)
            hipLaunchKernelGGL(k_shape_reduce_risk<1>, per_thread, dim3(256), 0, e->stream, d, gd, e->en, e->sh, e->risk_pi);
        else hipLaunchKernelGGL(k_shape_reduce_risk<64>, per_wave, dim3(256), 0, e->stream, d, gd, e->en, e->sh, e->risk_pi);
        return;
    }
    if (!e->shaped) hipLaunchKernelGGL(k_ens_reduce, per_thread, dim3(256), 0, e->stream, d, gd, e->en);
    else if (e->sh.col_band <= QOC_SHAPE_WAVE_FROM)
        hipLaunchKernelGGL(k_shape_reduce<1>, per_thread, dim3(256), 0, e->stream, d, gd, e->en, e->sh);
    else hipLaunchKernelGGL(k_shape_reduce<64>, per_wave, dim3(256), 0, e->stream, d, gd, e->en, e->sh);
}
// f(std::true_type) or f(std::false_type): a run-time flag as a template argument of what f launches
template <typename F>
static inline void with_flag(bool flag, F&& f) { flag ? f(std::true_type{}) : f(std::false_type{}); }
// 4. the tail on the view td that holds the control sets (the latency mode's fused tail runs in the last workgroup of its gradient kernel
// instead, with the local pulse regularisers too -- amplitude, envelope, dwdt, d2wdt2; the bandpass DFT keeps its own launches)
static void enqueue_tail(const qoc_engine* e, const QocDev& td, const QocAdamDev& ap, TailKind tail) {
    if (td.has_band) {
        const size_t items = (size_t)td.B * td.k * td.steps;
        hipLaunchKernelGGL(k_band_spectrum, dim3(grid_for(items, 4, 8192)), dim3(256), 0, e->stream, td);
        hipLaunchKernelGGL(k_band_gradient, dim3(grid_for(items, 256, 8192)), dim3(256), 0, e->stream, td);
    }
    const bool plain = !(td.has_amp || td.has_env || td.has_dwdt || td.has_d2wdt2 || td.has_band);
    with_flag(plain, [&](auto plain_c) {
        constexpr bool PLAIN = decltype(plain_c)::value;
        // control sets of 4097 .. 8192 (k, t) elements (C3: 6 x 1000) over fin_S workgroups in two launches: one set of 6000 elements
        // is bound by the fp64 sin / cos / sqrt / divide of the ONE compute unit k_finish_t runs it on (C3, one trajectory: 32.5 us;
        // profiles/r06_kernel_stats_c3_single_trajectory.txt)
        if (tail == TAIL_SPLIT || tail == TAIL_SPLIT_PARTIALS) {
            const dim3 sg((unsigned)e->fin_S, (unsigned)td.B);
            // (GEMM path, persistent chains: the wide gradient product left per-tile partial dots -- qoc_gemm_backward skipped its reduce
            // launch, part A sums them)
            QocGradPartial gp{nullptr, 0, 0, 0};
            if (tail == TAIL_SPLIT_PARTIALS) gp = QocGradPartial{e->gm.partial, e->gm.N / 32, e->gm.ldW, e->gm.MV};
            hipLaunchKernelGGL(k_finish_split_a<PLAIN>, sg, dim3(256), 0, e->stream, td, ap, e->fin_part, gp);
            hipLaunchKernelGGL(k_finish_split_b<PLAIN>, sg, dim3(256), 0, e->stream, td, ap, e->fin_part);
        } else with_flag(tail == TAIL_FINISH8, [&](auto wide_c) {   // ... or their Adam slots in registers too: eight elements per thread
            const dim3 fb(td.k * td.steps >= 2048 ? 1024 : QOC_BLOCK);
            hipLaunchKernelGGL((k_finish_t<PLAIN, decltype(wide_c)::value ? 8 : QF_E>), dim3(td.B), fb, 0, e->stream, td, ap);
        });
    });
}

static int enqueue_iteration(qoc_engine* e, const QocAdamDev& ap) {
    if (e->path == QOC_PATH_SMALL) return enqueue_small(e, ap, 1);
    const TailKind tail = tail_kind(e);
    const int skip = e->skip_mask;
    const bool own_controls = e->path == QOC_PATH_MFMA && e->mp.own_controls;
    const bool swap_in = e->controls_ready && !own_controls && !(skip & 1);
    QocDev& cv = sets(e);                    // (an ensemble: the group view holds the controls of the control sets)
    if (swap_in) { std::swap(cv.u, cv.u2); std::swap(cv.w, cv.w2); }
    e->controls_ready = false;
    QocDev d = e->d;
    if (own_controls) { d.u2 = nullptr; d.w2 = nullptr; }
    d.skip_done = ap.mode == 1 ? 1 : 0;      // qoc_eval / explicit steps always evaluate every seed
    d.uscale_in_loss = (e->path == QOC_PATH_MFMA && e->mp.uscale_in_loss) ? 1 : 0;
    QocDev gd = e->g;
    gd.skip_done = d.skip_done;
    const bool fused_tail = tail == TAIL_LATENCY_FUSED;
    // a control map: the member glue reads and writes the pulse view; k_map_expand / k_map_reduce join it and the trajectories
    QocDev pd = e->pv;
    pd.skip_done = d.skip_done;
    const QocDev& mv = e->mapped ? pd : d;
    const dim3 mapg_e(grid_for((size_t)d.B * d.k * d.steps, QOC_BLOCK, 2048)), mapg_r(grid_for((size_t)d.B * e->cm.k * d.steps, QOC_BLOCK, 2048));
    enqueue_controls(e, mv, gd, own_controls, swap_in);
    if (e->mapped && !(skip & 1)) hipLaunchKernelGGL(k_map_expand, mapg_e, dim3(QOC_BLOCK), 0, e->stream, d, pd, e->cm);
    TRY(enqueue_trajectories(e, d, ap, tail));
    if (e->mapped && !(skip & 32)) hipLaunchKernelGGL(k_map_reduce, mapg_r, dim3(QOC_BLOCK), 0, e->stream, d, pd, e->cm);
    if (e->ens_E && !(skip & 32)) enqueue_ens_reduce(e, mv, gd);
    if (!fused_tail && !(skip & 32)) enqueue_tail(e, e->ens_E ? gd : d, ap, tail);
    HIP_TRY(hipGetLastError());
    e->evaluated = true;
    // the Adam tail ran: u2 / w2 belong to the moved variable
    e->controls_ready = ap.mode != 0 && !own_controls && !(skip & (16 | 32));
    // final_state / unitary_scale are formed when read back
    e->final_stale = (e->path == QOC_PATH_MFMA && e->mp.final_on_readback) ||
                     (e->path == QOC_PATH_GEMM && e->gm.ts_G <= 0 && qoc_gemm_lazy_final(e->gm, e->d));
    // inter_vecs too, unless the batch kernels' source recursion needed them anyway
    e->inter_stale = e->path == QOC_PATH_MFMA && e->mp.inter_on_readback;          // (k_mfma_downup stores no Psi_t either)
    return QOC_OK;
}

// latency mode of the MFMA path: final_state and unitary_scale of the last evaluation, formed on demand
// workgroup-resident path: inter_vecs, final_state and unitary_scale of the last evaluation, re-formed from its controls (d.u) by the any-size kernels
static int refresh_small(qoc_engine* e, bool need_inter) {
    if (!e->final_stale && !(need_inter && e->inter_stale)) return QOC_OK;
    // unitary mode: the launch itself leaves final_state and unitary_scale of its last evaluation (from the root of its product tree), unless a deferred stop rule
    // undid that evaluation's successor; inter_vecs are always re-formed here
    if (!need_inter && !e->d.state_transfer && qoc_small_final_valid(e->sm, e->stream)) { e->final_stale = false; return QOC_OK; }
    QocDev d = e->d;
    d.skip_done = 0;
    if (!d.state_transfer) {
        hipLaunchKernelGGL(k_expm_generic, dim3(e->expm_grid), dim3(QOC_BLOCK), 0, e->stream, d, e->K, e->expm_scratch);
        hipLaunchKernelGGL(k_fwd_generic, dim3(d.B), dim3(QOC_BLOCK), 0, e->stream, d, e->K, e->seed_scratch);
    } else {
        hipLaunchKernelGGL(k_st_fwd_generic, dim3(d.B), dim3(QOC_BLOCK), 0, e->stream, d, e->seed_scratch);
        qoc_mfma_uscale_state_transfer(d, e->stream);
    }
    HIP_TRY(hipGetLastError());
    e->final_stale = false;
    e->inter_stale = false;
    return QOC_OK;
}

// several workgroups per control set: a spin on another workgroup's flag that gave up (it never should) left garbage behind -- say so
static int small_check(qoc_engine* e) {
    if (e->path != QOC_PATH_SMALL || e->sm.G <= 1) return QOC_OK;
    unsigned err = 0;
    HIP_TRY(hipMemcpy(&err, e->sm.sd.err, sizeof err, hipMemcpyDeviceToHost));
    if (err) return fail(QOC_ERR_HIP, "workgroup-resident iteration: an exchange between the %d workgroups of a control set timed out (are all %d workgroups "
        "resident?)", e->sm.G, e->sm.G * e->d.B);
    return QOC_OK;
}

static int refresh_final(qoc_engine* e) {
    if (e->path == QOC_PATH_SMALL) return refresh_small(e, false);
    if (!e->final_stale) return QOC_OK;
    // the boundary chain once more, with X beside the vectors
    if (e->path == QOC_PATH_GEMM) qoc_gemm_forward(e->gm, e->d, e->stream, true);
    else if (e->d.state_transfer) {                                                    // no final_state; unitary_scale from Psi_N
        if (e->inter_stale) { qoc_mfma_unpack_inter(e->mp, e->mf, e->d, e->stream); e->inter_stale = false; }
        qoc_mfma_uscale_state_transfer(e->d, e->stream);
    }
    else if (e->mp.final_from_groups) qoc_mfma_final_state(e->mp, e->mf, e->d, e->stream);
    else qoc_mfma_final_state_batch(e->mp, e->mf, e->d, e->stream);
    HIP_TRY(hipGetLastError());
    e->final_stale = false;
    return QOC_OK;
}

static QocAdamDev loop_params(const qoc_adam_params* p) {
    QocAdamDev ap;
    ap.mode = 1;
    ap.rate = p->rate;
    ap.decay = p->learning_rate_decay;
    ap.conv_target = p->conv_target;
    ap.min_grad = p->min_grad;
    ap.max_iterations = p->max_iterations;
    ap.lr = nullptr;
    return ap;
}

// ---- device-resident L-BFGS loop (csrc/qoc_lbfgs.h) ---------------------------------------------------------------------------------------
// history, direction and flags of every control set back to "no step taken" (the vectors need no clearing: no slot is live)
static int lbfgs_reset(qoc_engine* e) {
    const QocLbfgsDev& L = e->lq;
    const size_t B = (size_t)sets(e).B, R = 2 * (size_t)L.M + 1;
    HIP_TRY(hipMemsetAsync(L.st, 0, B * 8 * sizeof(int), e->stream));
    HIP_TRY(hipMemsetAsync(L.sc, 0, B * 4 * sizeof(double), e->stream));
    HIP_TRY(hipMemsetAsync(L.gram, 0, B * R * R * sizeof(double), e->stream));
    return QOC_OK;
}

// checks the parameters of a loop call (`who` names it), allocates the state on the first call (or for a longer history) and resets it when the history changes
static int lbfgs_prepare(qoc_engine* e, const qoc_lbfgs_params* p, const char* who, QocLbfgsDev* out) {
    if (!p) return fail(QOC_ERR_INVALID, "%s: null params", who);
    if (p->history < 1 || p->history > QOC_LBFGS_MAX_M) return fail(QOC_ERR_INVALID, "%s: history = %d, expected 1 .. %d", who, p->history, QOC_LBFGS_MAX_M);
    if (!(p->c1 > 0.0 && p->c1 < 1.0)) return fail(QOC_ERR_INVALID, "%s: c1 = %g, expected a value in (0, 1)", who, p->c1);
    if (!(p->shrink > 0.0 && p->shrink < 1.0)) return fail(QOC_ERR_INVALID, "%s: shrink = %g, expected a value in (0, 1)", who, p->shrink);
    if (p->max_ls < 1) return fail(QOC_ERR_INVALID, "%s: max_ls = %d, expected >= 1", who, p->max_ls);
    if (e->cfg.time_shards > 0 || e->gm.ts_G > 0)
        return fail(QOC_ERR_INVALID, "%s: the L-BFGS loop does not run on a time-sharded engine (every rank would have to take the same line-search decisions)", who);
    const QocDev& sd = sets(e);
    const size_t B = (size_t)sd.B, N = (size_t)sd.k * sd.steps;
    QocLbfgsDev& L = e->lq;
    // The small arrays once, for the longest history.  The vectors for the history asked for first (what most engines ever use); a later, longer history takes
    // ONE new block for QOC_LBFGS_MAX_M pairs -- the arena cannot give the first block back, so an engine holds at most these two until qoc_destroy, however
    // the histories of later calls alternate.  The vectors come last: a QOC_ERR_NOMEM leaves nothing but the few KB of the small arrays behind.
    if (!L.gram) {
        const size_t R = QOC_LBFGS_ROWS;
        TRY(dev_alloc(e, &L.gram, B * R * R));
        TRY(dev_alloc(e, &L.sc, B * 4));
        TRY(dev_alloc(e, &L.st, B * 8));
    }
    if (!L.vec || p->history > e->lq_cap) {
        const size_t M = L.vec ? (size_t)QOC_LBFGS_MAX_M : (size_t)p->history;
        double* vec = nullptr;
        TRY(dev_alloc(e, &vec, B * (2 * M + 3) * N));
        // (on the engine's stream, as every later use: the null stream orders nothing against it)
        HIP_TRY(hipMemsetAsync(vec, 0, B * (2 * M + 3) * N * sizeof(double), e->stream));
        L.vec = vec;
        L.M = 0;
        e->lq_cap = (int)M;
    }
    L.N = (int)N;
    if (L.M != p->history) {
        L.M = p->history;
        TRY(lbfgs_reset(e));
    }
    L.conv_target = p->conv_target; L.min_grad = p->min_grad; L.c1 = p->c1; L.shrink = p->shrink;
    L.max_iterations = p->max_iterations; L.max_ls = p->max_ls;
    *out = L;
    return QOC_OK;
}

// one loop iteration: the evaluate-only iteration of qoc_eval, then the step on the view that holds the control sets
static int enqueue_lbfgs_iteration(qoc_engine* e, const QocLbfgsDev& L) {
    QocAdamDev ap;
    memset(&ap, 0, sizeof ap);
    ap.mode = 0;
    TRY(enqueue_iteration(e, ap));
    const QocDev& sd = sets(e);
    hipLaunchKernelGGL(k_lbfgs_step, dim3(sd.B), dim3(L.N >= 2048 ? 1024 : QOC_BLOCK), 0, e->stream, sd, L);
    HIP_TRY(hipGetLastError());
    e->controls_ready = false;                 // the variable moved on the device: u2 / w2 are not its controls
    return QOC_OK;
}

// the poll loop of qoc_run_adam and qoc_run_lbfgs (`who`): bursts of poll_every evaluations, the last one cut to the budget; after each the stream
// is drained and the stop flags are read, until every control set has stopped (`what` names them in the failure message)
template <typename F>
static int run_until_done(qoc_engine* e, const char* who, const char* what, long long budget, int poll_every, int32_t* iterations_out,
                          F&& enqueue_burst) {
    const int poll = poll_every > 0 ? poll_every : 1;
    const QocDev& sd = sets(e);
    std::vector<int> done(sd.B);
    long long launched = 0;
    while (true) {
        int burst = poll;
        if (launched + burst > budget) burst = (int)(budget - launched);
        TRY(enqueue_burst(burst));
        launched += burst;
        HIP_TRY(hipStreamSynchronize(e->stream));
        TRY(small_check(e));
        HIP_TRY(hipMemcpy(done.data(), sd.done, sd.B * sizeof(int), hipMemcpyDeviceToHost));
        bool all = true;
        for (int b = 0; b < sd.B; ++b) all = all && done[b];
        if (all) break;
        if (launched >= budget) return fail(QOC_ERR_STATE, "%s: %s not finished after %lld evaluations", who, what, launched);
    }
    if (iterations_out) HIP_TRY(hipMemcpy(iterations_out, sd.iters, sd.B * sizeof(int), hipMemcpyDeviceToHost));
    return QOC_OK;
}


// the response matrix of qoc_create_shaped as the host prepared it: the transposed copy and the nonzero window of every row and column
struct ShapeHost {
    int P, band, col_band;
    std::vector<double> Tt;          // [P][steps]: T transposed (what the kernels read)
    std::vector<int2> row_win, col_win;
};

// what qoc_create_ensemble adds to the trajectory engine it creates: the caller's own configuration (k controls, n_seeds control sets, the
// pulse regularisers) for the group view, and the member description
struct EnsArgs {
    const qoc_config* user;
    const double* maxA;              // [k]
    const double* one_minus_gauss;   // [k][steps] or null
    const qoc_ensemble* ens;
    const ShapeHost* shape;          // qoc_create_shaped: the response matrix and its windows, else null
    const qoc_control_map* map;      // qoc_create_mapped: the checked map, else null
    const qoc_fleet* fleet;          // qoc_create_fleet: the checked member tables of the F devices (in place of ens' offsets and amp_scales), else null
};

// the decay of an open engine: the collapse operators and, on an ensemble or fleet (qoc_create_open_fleet), the rate scales of every member
struct DecayHost {
    int c;
    const double* C;                 // [c][n][n] complex: sqrt(dt) C_j at scale 1
    const double* scales;            // [F][E][c] or null (ones)
    int F, E;                        // the rows of `scales` (1, 1: qoc_create_open)
    const char* who;
    const qoc_running_costs* costs = nullptr;   // qoc_create_open_costs: the checked running costs (n_obs > 0), else null
};

// the operators of qoc_create_sparse as the host prepared them: one ELLPACK block per operator (csrc/qoc_sparse_host.h)
// (qoc_create_sparse_fleet: kt + q + 1 operators, the merged layout of them when the sweeps walk it, and kt, the rows k_sp_grad forms gradients for)
struct SparseHost {
    std::vector<QocEllOp> ops;       // [k+1]
    int vector_home;
    const char* who = "qoc_create_sparse";
    int kgrad = -1;                  // -1: every row (qoc_create_sparse)
    bool fleet_entry = false;        // made by qoc_create_sparse_fleet: the plan string names the row layout
    bool merged = false;
    QocMergedOps rows;               // merged only
};

// the caller's arrays of qoc_create (include/qoc.h), passed on together (sparse: the operators of qoc_create_sparse in place of Hs, else null)
struct Problem {
    const double *Hs, *U0, *V, *W, *maxA, *one_minus_gauss; const int32_t* forbidden_states; const double *forbidden_coeffs, *Vs;
    const SparseHost* sparse;
    const DecayHost* decay;          // an open engine (qoc_create_open, qoc_create_open_fleet, qoc_create_open_costs), else null
};

static int check_create_args(const qoc_config* cfg, const Problem& p, qoc_handle* out) {
    if (!cfg || (!p.Hs && !p.sparse) || !p.V || !p.W || !p.maxA || !out) return fail(QOC_ERR_INVALID, "qoc_create: null argument");
    if (cfg->plan_seeds < 0)
        return fail(QOC_ERR_INVALID, "qoc_create: plan_seeds = %d (0 = plan for n_seeds, > 0 = the batch AUTO plans for)", cfg->plan_seeds);
    if (cfg->n < 1 || cfg->k < 1 || cfg->steps < 1 || cfg->m < 1 || cfg->n_seeds < 1)
        return fail(QOC_ERR_INVALID, "qoc_create: n, k, steps, m, n_seeds must be >= 1");
    if (cfg->taylor_terms < 1 || cfg->scaling < 0 || cfg->scaling > 30)
        return fail(QOC_ERR_INVALID, "qoc_create: bad taylor_terms/scaling (%d, %d)", cfg->taylor_terms, cfg->scaling);
    if (!cfg->state_transfer && !p.U0) return fail(QOC_ERR_INVALID, "qoc_create: U0 required in unitary mode");
    if (cfg->n_forbidden < 0) return fail(QOC_ERR_INVALID, "qoc_create: n_forbidden must be >= 0");
    if (cfg->n_forbidden > 0 && (!p.forbidden_states || !p.forbidden_coeffs))
        return fail(QOC_ERR_INVALID, "qoc_create: forbidden lists missing");
    if (cfg->forbid_dressed && cfg->n_forbidden > 0 && !p.Vs) return fail(QOC_ERR_INVALID, "qoc_create: forbid_dressed needs Vs");
    if (cfg->has_envelope && !p.one_minus_gauss) return fail(QOC_ERR_INVALID, "qoc_create: envelope constant missing");
    if (cfg->has_d2wdt2 && !cfg->has_dwdt) return fail(QOC_ERR_INVALID, "qoc_create: d2wdt2 needs dwdt (reference: NameError new_weights)");
    for (int f = 0; f < cfg->n_forbidden; ++f)
        if (p.forbidden_states[f] < 0 || p.forbidden_states[f] >= cfg->n)
            return fail(QOC_ERR_INVALID, "qoc_create: forbidden state %d out of range", p.forbidden_states[f]);
    if (cfg->gradient != 0 && cfg->gradient != 1)
        return fail(QOC_ERR_INVALID, "qoc_create: gradient = %d (0 = first-order, the reference's; 1 = exact gradient)", cfg->gradient);
    if (cfg->gradient == 1) {
        // the exact gradient runs behind the generic path's forward (csrc/qoc_exact_grad.h); the other paths keep K_t in layouts of their own
        if (cfg->path != QOC_PATH_AUTO && cfg->path != QOC_PATH_GENERIC)
            return fail(QOC_ERR_INVALID, "qoc_create: the exact gradient runs on the generic path (QOC_PATH_GENERIC or AUTO), not on path %d", cfg->path);
        if (cfg->time_shards > 0)
            return fail(QOC_ERR_INVALID, "qoc_create: the exact gradient cannot be time-sharded (time_shards = %d)", cfg->time_shards);
    }
    int ndev = 0;
    const hipError_t de = hipGetDeviceCount(&ndev);
    if (de != hipSuccess || ndev == 0)
        return fail(QOC_ERR_HIP, "qoc_create: no HIP device visible (%s) -- this engine has no CPU fallback",
                    de == hipSuccess ? "count = 0" : hipGetErrorString(de));
    if (cfg->device < 0 || cfg->device >= ndev) return fail(QOC_ERR_INVALID, "qoc_create: device %d of %d", cfg->device, ndev);
    return QOC_OK;
}

// the pulse regularisers of a view that holds control sets, per slice (a sample view: per sample) of that view
static void fill_pulse_regularisers(QocDev& v, const qoc_config& c) {
    const double inv_steps = 1.0 / (double)v.steps;
    v.has_amp = c.has_amplitude; v.a_amp = c.c_amplitude * inv_steps;
    v.has_env = c.has_envelope; v.a_env = c.c_envelope * inv_steps;
    v.has_dwdt = c.has_dwdt; v.a_dwdt = c.c_dwdt * inv_steps;
    v.has_d2wdt2 = c.has_d2wdt2; v.a_d2wdt2 = c.c_d2wdt2 * inv_steps;
    v.has_band = c.has_bandpass; v.a_band = c.c_bandpass * inv_steps;
    v.band_lo = c.band_lo; v.band_hi = c.band_hi;
}
// U0 V (state transfer: V itself): the start vectors of the thin forward recursion
static std::vector<double> start_vectors(const qoc_config& c, const double* U0, const double* V) {
    const int n = c.n, m = c.m;
    std::vector<double> psi0(V, V + 2 * (size_t)n * m);
    if (c.state_transfer) return psi0;
    for (int a = 0; a < n; ++a)
        for (int j = 0; j < m; ++j) {
            double re = 0, im = 0;
            for (int l = 0; l < n; ++l) {
                const double ur = U0[2 * (a * n + l)], ui = U0[2 * (a * n + l) + 1];
                const double vr = V[2 * (l * m + j)], vi = V[2 * (l * m + j) + 1];
                re += ur * vr - ui * vi;
                im += ur * vi + ui * vr;
            }
            psi0[2 * (a * m + j)] = re; psi0[2 * (a * m + j) + 1] = im;
        }
    return psi0;
}

// ---- the state of a view that holds control sets: e->d of a plain engine, e->g of an ensemble engine (whose e->d keeps its own, unused by
// the tail).  Three helpers because a plain engine allocates its trajectory buffers between them, and the arena is a bump allocator whose
// layout the measurements were taken on.  `who`: the entry point that builds the view.  First the variable, Adam slots, stop rule, controls
// and gradients, and -- tail_here: the tail runs on this view -- above 4096 (k, t) elements the partials of the split tail over fin_S
// workgroups per control set (k_finish_split_a / _b; the switch: A/B runs)
static int alloc_set_arrays(qoc_engine* e, QocDev& v, const char* who, bool tail_here) {
    const size_t B = (size_t)v.B, ks = (size_t)v.k * v.steps, all = B * ks;
    for (double** p : {&v.base, &v.adam_m, &v.adam_v}) TRY(dev_zalloc(e, p, all, who));
    for (int** p : {&v.adam_t, &v.iters, &v.done}) TRY(dev_zalloc(e, p, B, who));
    for (double** p : {&v.w, &v.u, &v.w2, &v.u2, &v.dLdu, &v.grad}) TRY(dev_alloc(e, p, all));
    if (!tail_here || ks <= 4 * 1024 || qoc_exp_is("QOC_FINISH_SPLIT", 0)) return QOC_OK;
    e->fin_S = (int)grid_for(ks, 256, 64);                         // (longer pulses: several elements per thread)
    return dev_alloc(e, &e->fin_part, B * (e->fin_S + 2) * 2);
}
// the scalars of every control set and the arrays of the bandpass regulariser with its phase table (no_table: the message without one)
static int alloc_set_scalars(qoc_engine* e, QocDev& v, const char* who, const char* no_table) {
    const size_t B = (size_t)v.B, all = B * v.k * v.steps;
    for (double** p : {&v.loss, &v.reg_state, &v.reg_loss, &v.g2}) TRY(dev_alloc(e, p, B));
    TRY(dev_zalloc(e, &v.uscale, B, who));
    if (!v.has_band) return QOC_OK;
    TRY(dev_alloc(e, &v.band_ph, all)); TRY(dev_alloc(e, &v.band_tw, (size_t)v.steps));
    TRY(dev_alloc(e, &v.band_mag, all)); TRY(dev_alloc(e, &v.band_dR, all));
    hipLaunchKernelGGL(k_band_twiddles, dim3((v.steps + 255) / 256), dim3(256), 0, 0, v.band_tw, v.steps);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(0) != hipSuccess) return fail(QOC_ERR_HIP, "%s", no_table);
    return QOC_OK;
}
static int build_trajectory_view(qoc_engine* e, const Problem& p) {
    const qoc_config& c = e->cfg;
    QocDev& d = e->d;
    const size_t B = (size_t)d.B, pts = B * (d.steps + 1), nn = (size_t)d.n * d.n, nm = (size_t)d.n * d.m;
    const std::vector<double> psi0 = start_vectors(c, p.U0, p.V);
    // a sparse engine holds no n x n array, on the host or on the device: d.Hs, d.U0 and d.Xfinal stay null (no kernel of its path reads them)
    if (!p.sparse) {
        std::vector<double> ident(p.U0 ? 0 : 2 * nn, 0.0);         // (state transfer without a start unitary)
        if (!p.U0) for (int a = 0; a < c.n; ++a) ident[2 * (a * c.n + a)] = 1.0;
        TRY(dev_upload(e, &d.Hs, (const cplx*)p.Hs, (size_t)(c.k + 1) * nn));
        TRY(dev_upload(e, &d.U0, (const cplx*)(p.U0 ? p.U0 : ident.data()), nn));
    }
    TRY(dev_upload(e, &d.V, (const cplx*)p.V, nm)); TRY(dev_upload(e, &d.W, (const cplx*)p.W, nm));
    TRY(dev_upload(e, &d.Psi0, (const cplx*)psi0.data(), nm));
    if (d.forbid_dressed) TRY(dev_upload(e, &d.Vs, (const cplx*)p.Vs, nn));
    TRY(dev_upload(e, &d.maxA, p.maxA, (size_t)c.k));
    if (p.one_minus_gauss) TRY(dev_upload(e, &d.omg, p.one_minus_gauss, (size_t)c.k * c.steps));
    if (c.n_forbidden > 0) {
        std::vector<double> fa(c.n_forbidden);
        for (int f = 0; f < c.n_forbidden; ++f) fa[f] = p.forbidden_coeffs[f] * (1.0 / (double)c.steps);
        TRY(dev_upload(e, &d.forb_state, (const int*)p.forbidden_states, (size_t)c.n_forbidden));
        TRY(dev_upload(e, &d.forb_a, (const double*)fa.data(), (size_t)c.n_forbidden));
    }
    TRY(alloc_set_arrays(e, d, "qoc_create", !e->ens_E));         // (an ensemble runs the tail on its group view)
    TRY(dev_alloc(e, &d.inter, pts * nm));
    if (!p.sparse) TRY(dev_zalloc(e, &d.Xfinal, B * nn, "qoc_create"));
    TRY(dev_alloc(e, &d.ztau, pts));
    if (d.n_forb > 0) TRY(dev_alloc(e, &d.Fpop, pts * d.n_forb * d.m));
    if (d.forbid_dressed && d.n_forb > 0) TRY(dev_alloc(e, &d.Fd, pts * d.n_forb * d.m));
    TRY(dev_alloc(e, &d.zfin, B)); TRY(dev_zalloc(e, &d.su_resid, B, "qoc_create"));
    TRY(alloc_set_scalars(e, d, "qoc_create", "qoc_create: the phase table of the bandpass regulariser could not be formed"));
    return dev_alloc(e, &e->step_lr, B);
}

struct AutoPlan { int path; bool latency, gemm_direct, mfma_ok, st_ok, gemm_ok; };     // (.._ok: the path can run the problem at all)

// The batch-size-dependent part of AUTO as a function of the batch Bp it plans for (tests/test_auto_plan.py restates this table row by row)
// Every batch-size-dependent choice is taken for Bp = qoc_config.plan_seeds (else the local batch): a shard of a restart batch then runs
// the same path, kernels and chunking as the whole batch would.
//
// Measured with tools/path_sweep.py (profiles/r01_path_sweep.txt):
//  * unitary, n <= 32: the register-resident MFMA chain kernels win on throughput (1.8 vs 2.3 ms per iteration of 64 C2 seeds), the GEMM
//    path (fused LDS-resident exponential + product tree + persistent thin chains) on latency (0.19 vs 0.47 ms for one C2 trajectory; level
//    at 12 seeds, 0.56 vs 0.49 ms at 16 since the batch kernels split the pulse into up to 64 chunks: profiles/r02_latency_sweep.txt); 32 <
//    n <= 48 (NT = 3: exponentials by three waves per item on v_mfma_f64_4x4x4, costate sweep + slice-parallel gradient kernel): the MFMA
//    path wins from 8 seeds on (1.11 vs 1.50 ms at 8, 1.70 vs 2.72 at 16, 5.27 vs 9.88 ms at 64 seeds of n = 48; the GEMM path pads to N =
//    64), ties at 4 (1.00 vs 0.95) and loses below (0.96 vs 0.62 ms at 2); 48 < n <= 64 (NT = 4; tools/n64_batch_sweep.py): with k <= 4
//    controls the MFMA path is ahead from 32 seeds on (4.96 vs 5.14 ms at 32, 9.16 vs 10.05 at 64, 17.4 vs 19.8 at 128 seeds of n = 64 x
//    500 slices, since the row-tile gradient kernel); with more controls the GEMM path up to 64 seeds, the MFMA path beyond (since
//    k_mfma_expm_rows lost its scratch: k = 6 x 200 slices 4.33 vs 4.35 ms at 64 seeds, 7.86 vs 8.47 at 128; k = 8 x 1000 slices 20.05 vs
//    20.54 at 64, 38.7 vs 40.7 at 128; at 32 seeds the GEMM path: 2.31 vs 2.59, 10.4 vs 10.7).
//  * a handful of control sets of an n <= 32 unitary problem (the reference's own use is ONE per Grape() call): the latency mode of the
//    MFMA path. It spends a workgroup per time slice, so what decides is seeds x slices (profiles/r02_latency_sweep.txt,
//    r02_small_n_sweep.txt): C2 (500 slices) 0.083 ms against 0.189 (GEMM route) and 0.56 (batch kernels) for one seed, still ahead at 12
//    seeds, level at 16; n <= 16 is padded to 32 and competes with the cheap NT = 1 batch kernels: ahead up to 4 seeds (n = 16 x 500
//    slices: 0.081 against 0.203 ms for one seed, 0.163 against 0.213 for four) (with k_mfma_expm_slice2 on the active strips: ahead up to
//    6 control sets with or without a state regulariser -- n = 16 x 500 slices x 6: 0.180 against 0.213 ms, with a forbidden level 0.250
//    against 0.280; x 8: 0.229 / 0.213 and 0.308 / 0.280; n = 9 x 300 x 6: 0.106 / 0.140; profiles/r04_small_n_latency.txt) 32 < n <= 48
//    (NT = 3 kernels: k_mfma_expm_rows per slice, the same chains, sweeps and gradient): one trajectory of n = 48 x 500 slices 0.165 ms
//    against 0.454 (GEMM route) and 0.84 (batch kernels); ahead up to 8 seeds (profiles/r02_mid_n_sweep.txt). With a state regulariser
//    (forbidden levels, speed_up: lat_src) the backward half is the affine recursion of the batch kernels on the latency mode's chunks,
//    with two-level boundaries (QocMfma::lat_sources): one C2 trajectory with dwdt + forbidden levels 0.189 ms against 0.290 (GEMM route)
//    and 0.72 (batch kernels); ahead up to ~4096 seed-slices (tools/c2_forbidden_single.py).
//  * n > 32 with ONE state vector (dpp_shape): the direct route runs k_gemm_taylor_chain_dpp (0.31 against 0.46 us per dependent mat-vec)
//    and wins earlier -- C3 (n = 64, k = 6, 1000 slices), propagator / direct route in ms: x 24 6.03 / 6.20, x 32 8.00 / 6.34; without
//    forbidden levels (both chains side by side) x 12 2.81 / 3.12, x 16 3.74 / 3.18 (profiles/r04_c3_route_sweep.txt); n = 40, 48 with k =
//    4 x 500 slices, MFMA batch kernels / direct: x 24 1.48 / 1.64, x 32 1.84 / 1.70; with forbidden levels x 32 2.14 / 3.20, x 48 3.89 /
//    3.32 (profiles/r04_st_direct_sweep.txt). Three-multiplication form of the DPP chain, profiles/r04_c3_route_sweep_gauss.txt: with
//    forbidden levels x 20 5.05 / 5.43, x 22 5.56 / 5.45, x 24 6.02 / 5.49; without x 11 2.63 / 2.77, x 12 2.84 / 2.79, x 13 3.11 / 2.81 --
//    the limits (ST_DIRECT_FROM) moved from 28 / 14 to 22 / 12.
//  * state transfer on the MFMA path (tools/st_path_sweep.py -> profiles/r04_state_transfer_paths.txt; m = 1, T = 10, 500 slices, ms per
//    iteration, GEMM path / MFMA batch kernels / latency mode): n = 32 x 1: 0.125 / 0.300 / 0.073, x 4: 0.159 / 0.304 / 0.143, x 16: 0.388
//    / 0.324, x 64: 1.30 / 0.99, x 256: 2.00 (direct Taylor chains) / 3.78; n = 16 x 1: 0.126 / 0.192 / 0.063, x 8: 0.219 / 0.209 / 0.203,
//    x 64: 1.28 / 0.34, x 256: 1.94 / 1.16; n = 48 x 1: 0.245 / 0.72 / 0.120, x 8: 1.02 / 0.77 / 0.58, x 16: 1.87 / 1.11, x 64: 2.60 / 3.31
//    (with forbidden levels 4.85 / 4.00); n = 64 (C3: k = 6, 1000 slices) x 1: 0.417 / 3.0 / 0.449, x 64: 9.73 / 18.1 -- so (mfma_auto):
//    the unitary table for n <= 32 and for 32 < n <= 48 with k <= 4 (NT = 3), the latency mode of n <= 16 up to 8 control sets and from 25
//    levels on up to 4, the GEMM route for up to 8 control sets from 25 levels on, and the direct Taylor chains of the GEMM path for the
//    large batches they win (n <= 32: from 112 control sets of more than 20 levels, 28 with a state regulariser; n > 32: from 48, 112).
static AutoPlan plan_for(const qoc_config& cfg, const QocDev& d, bool antiherm, bool ensemble, int Bp) {
    const int n = cfg.n, k = cfg.k, steps = cfg.steps, m = cfg.m;
    const bool st = cfg.state_transfer != 0;
    // (state transfer: the propagator's adjoint is the reference's gradient only with anti-Hermitian generators)
    const bool mfma_ok = qoc_mfma_supported(d) && antiherm, gemm_ok = qoc_gemm_supported(d, antiherm);
    const bool st_ok = st_fused_supported(d), direct_ok = qoc_gemm_direct_supported(d);
    const bool lat_src = d.n_forb > 0 || d.has_speed;
    const bool dpp_shape = n > 32 && m == 1;
    const int ST_DIRECT_FROM = n <= 32 ? QOC_PLAN_ST_DIRECT_N32 : (dpp_shape ? (lat_src ? QOC_PLAN_ST_DIRECT_DPP_SRC
        : QOC_PLAN_ST_DIRECT_DPP) : QOC_PLAN_ST_DIRECT_N64);
    const bool mfma_auto = mfma_ok && (!st || n <= 32 || (n <= 48 && k <= 4));
    const bool nt4_batch = n > 48 && ((k <= 4 && Bp >= QOC_PLAN_NT4_MIN_SETS_K4) || Bp >= QOC_PLAN_NT4_MIN_SETS);
    // 16 < n <= 32 below the latency mode's reach (long pulses): the GEMM route up to a few control sets, fewer the smaller the active part
    // of the padded matrices is (500 slices, GEMM route / MFMA batch kernels in ms: n = 32 x 6 0.290 / 0.315, x 8 0.340 / 0.318; n = 27 x 4
    // 0.251 / 0.270, x 6 0.288 / 0.271; n = 20 x 2 0.185 / 0.196, x 4 0.249 / 0.196; with a forbidden level n = 32 x 8 0.436 / 0.473, n =
    // 27 x 8 level, n = 20 x 6 0.373 / 0.360)
    const int qa_g = (n + 3) / 4;
    const int gemm_small = (st && qa_g >= 7) ? QOC_PLAN_GEMM_SMALL_ST_WIDE
                           : lat_src ? (qa_g <= 5 ? QOC_PLAN_GEMM_SMALL_SRC_Q5 : qa_g == 6 ? QOC_PLAN_GEMM_SMALL_SRC_Q6
                               : QOC_PLAN_GEMM_SMALL_SRC_Q78)
                                     : (qa_g <= 5 ? QOC_PLAN_GEMM_SMALL_Q5 : qa_g == 6 ? QOC_PLAN_GEMM_SMALL_Q6 : qa_g == 7
                                         ? QOC_PLAN_GEMM_SMALL_Q7 : QOC_PLAN_GEMM_SMALL_Q8);
    const bool st_big = st && direct_ok && cfg.chunks <= 1 &&
                        (n <= 32 ? (Bp >= QOC_PLAN_ST_BIG_N32
                            && n > (lat_src ? QOC_PLAN_ST_BIG_N32_MIN_LEVELS_SRC : QOC_PLAN_ST_BIG_N32_MIN_LEVELS))
                                 : Bp >= (dpp_shape ? (lat_src ? QOC_PLAN_ST_BIG_DPP_SRC : QOC_PLAN_ST_BIG_DPP) : (lat_src
                                     ? QOC_PLAN_ST_BIG_N64_SRC : QOC_PLAN_ST_BIG_N64)));
    const bool prefer_gemm = gemm_ok && ((n > 48 && !nt4_batch) || (n > 32 && Bp < QOC_PLAN_NT3_MIN_SETS) ||
                                         (n > 16 && n <= 32 && Bp <= gemm_small && m <= 8 && steps >= QOC_PLAN_GEMM_SMALL_MIN_SLICES)
                                             || st_big);
    const long long lat_work = (long long)Bp * steps;
    // 16 < n <= 32: the batch kernels work on the ACTIVE 4-row strips qa = ceil(n / 4) of the padded matrices and take over earlier the
    // smaller n is (tools/padded_latency_sweep.py, 500 slices: n = 20 / 24 / 27 / 32 level at ~5 / 6 / 7 / 8.5 control sets; with a
    // forbidden level the latency mode stays ahead up to 8, at n = 20 up to 7): seeds x slices <= 512 qa, with a state regulariser
    // min(4096, 768 qa)
    const int qa = (n + 3) / 4 < 5 ? 5 : (n + 3) / 4;
    const long long lat_limit = n <= 16 ? (lat_src ? QOC_PLAN_LAT_WORK_SRC : QOC_PLAN_LAT_WORK)
                                        : (lat_src ? std::min<long long>(QOC_PLAN_LAT_WORK_SRC,
                                            (long long)QOC_PLAN_LAT_WORK_PER_STRIP_SRC * qa)
                                                   : (long long)QOC_PLAN_LAT_WORK_PER_STRIP * qa);
    // NT = 4 (also 32 < n <= 48 with k > 4, padded): 0.268 against 0.458 ms (GEMM route) for one seed of 500 slices, level at 8; NT = 3:
    // the competitors are slower (tools/mid_n_sweep.py); state transfer from 25 levels on: 5 .. 8 control sets go to the GEMM route -- n =
    // 32 x 8: 0.220 against 0.261 ms, with forbidden levels 0.272 / 0.316
    const int lat_sets = n > 16 ? ((st && qa_g >= 7) ? QOC_PLAN_LAT_SETS_N32_ST_WIDE : QOC_PLAN_LAT_SETS_N32) : (st
        ? QOC_PLAN_LAT_SETS_N16_ST : QOC_PLAN_LAT_SETS_N16);
    const bool latency = !ensemble && cfg.path == QOC_PATH_AUTO && cfg.variant == 0 && mfma_auto && qoc_mfma_latency_ok(d)
        && steps >= QOC_PLAN_LAT_MIN_SLICES &&
                          (((n > 48 || (n > 32 && k > 4)) ? (lat_work <= QOC_PLAN_LAT_WORK_NT4 && Bp <= QOC_PLAN_LAT_SETS_NT4)
                            : n > 32 ? (lat_work <= QOC_PLAN_LAT_WORK_NT3 && Bp <= QOC_PLAN_LAT_SETS_NT3)
                                     : (lat_work <= lat_limit && Bp <= lat_sets)) ||
                           (Bp == 1 && steps <= QOC_PLAN_LAT_SINGLE_MAX_SLICES));
    AutoPlan p;
    p.mfma_ok = mfma_ok; p.st_ok = st_ok; p.gemm_ok = gemm_ok;
    p.latency = latency;
    p.gemm_direct = direct_ok && (!antiherm || cfg.chunks == 1 || (cfg.chunks == 0 && Bp >= ST_DIRECT_FROM));
    p.path = cfg.path != QOC_PATH_AUTO ? cfg.path
             : latency ? QOC_PATH_MFMA : (mfma_auto
                 && !prefer_gemm) ? QOC_PATH_MFMA : (gemm_ok ? QOC_PATH_GEMM : (st_ok ? QOC_PATH_ST_FUSED : QOC_PATH_GENERIC));
    return p;
}

// the plan of this engine: plan_for its planned batch, then what overrides the table, then whether the path can run the problem at all
static int choose_path(const qoc_config& cfg, const QocDev& d, bool antiherm, bool ensemble, AutoPlan& plan) {
    const int n = cfg.n, k = cfg.k, m = cfg.m, B = cfg.n_seeds;
    if (cfg.state_transfer && cfg.path == QOC_PATH_GEMM && cfg.chunks > 1 && !antiherm)
        return fail(QOC_ERR_INVALID,
            "qoc_create: the propagator route of the GEMM path (chunks > 1) needs exactly anti-Hermitian generators");
    plan = plan_for(cfg, d, antiherm, ensemble, d.Bplan);
    if (d.Bplan < B && cfg.gradient != 1) {
        // a plan for FEWER control sets than the engine holds is legal (a rank that holds several shards of a planned batch keeps
        // bit-identity with them) but can cost a factor: say so once when it changes what AUTO would have picked for the resident batch
        const AutoPlan own = plan_for(cfg, d, antiherm, ensemble, B);
        if (own.path != plan.path || own.latency != plan.latency || own.gemm_direct != plan.gemm_direct)
            fprintf(stderr, "libqoc_hip: note: plan_seeds = %d < n_seeds = %d changes the AUTO plan (path %d%s instead of %d%s): kernels "
                "tuned for the smaller batch run on the larger one\n",
                    d.Bplan, B, plan.path, plan.latency ? " latency mode" : "", own.path, own.latency ? " latency mode" : "");
    }
    // n <= 12, one or a few control sets (the reference's own use) and small batches: the workgroup-resident iteration (csrc/qoc_small.h) --
    // 5-20 us per iteration where the paths above pay 42-57 us of launches and dependent round trips whatever n (profiles/r06_small_n_latency.txt)
    // (QOC_EXPERIMENTAL=1 QOC_SMALL_AUTO=0: AUTO without it, for A/B runs -- tools/small_n_latency.py)
    if (!ensemble && cfg.path == QOC_PATH_AUTO && cfg.variant == 0 && cfg.chunks == 0 && cfg.time_shards < 1
        && !qoc_exp_is("QOC_SMALL_AUTO", 0) && qoc_small_auto(d, antiherm))
        plan.path = QOC_PATH_SMALL;
    if (cfg.gradient == 1) plan.path = QOC_PATH_GENERIC;             // (whatever AUTO's table says: the exact gradient has one home)
    if (cfg.time_shards >= 1) {
        if (cfg.time_rank < -1 || cfg.time_rank >= cfg.time_shards)
            return fail(QOC_ERR_INVALID, "qoc_create: time_rank %d of %d time shards", cfg.time_rank, cfg.time_shards);
        if (cfg.path != QOC_PATH_AUTO && cfg.path != QOC_PATH_GEMM)
            return fail(QOC_ERR_INVALID, "qoc_create: time sharding runs on the GEMM path");
        plan.path = QOC_PATH_GEMM;
    }
    if (plan.path == QOC_PATH_MFMA && !plan.mfma_ok)
        return fail(QOC_ERR_INVALID, "qoc_create: MFMA path needs n <= 64, m <= 16, k <= 8, a Taylor degree of 1 .. 22 and, in state "
            "transfer, exactly anti-Hermitian generators (n=%d m=%d k=%d T=%d)", n, m, k, d.T);
    if (plan.path == QOC_PATH_ST_FUSED && !plan.st_ok)
        return fail(QOC_ERR_INVALID,
            "qoc_create: fused state-transfer path needs state_transfer, n <= 64, m <= 4, k <= 8 (n=%d m=%d k=%d)", n, m, k);
    if (plan.path == QOC_PATH_GEMM && !plan.gemm_ok)
        return fail(QOC_ERR_INVALID,
            "qoc_create: GEMM path needs m <= 32 and, in state transfer, exactly anti-Hermitian generators or n <= 64, m <= 8 (m=%d)", m);
    if (plan.path < QOC_PATH_GENERIC || plan.path > QOC_PATH_SMALL) return fail(QOC_ERR_INVALID, "qoc_create: unknown path %d", plan.path);
    return QOC_OK;
}

// the any-size kernels' buffers: the generic path's own, and the workgroup-resident path's for its read-backs
static int alloc_generic_scratch(qoc_engine* e) {
    const QocDev& d = e->d;
    const size_t B = (size_t)d.B, nn = (size_t)d.n * d.n, nm = (size_t)d.n * d.m;
    if (d.state_transfer) return dev_alloc(e, &e->seed_scratch, B * (nn + 3 * nm));
    TRY(dev_alloc(e, &e->K, B * d.steps * nn));
    e->expm_grid = (int)grid_for(B * d.steps, 1, 4096);
    TRY(dev_alloc(e, &e->expm_scratch, (size_t)e->expm_grid * 3 * nn));
    return dev_alloc(e, &e->seed_scratch, B * (2 * nn + 2 * nm));
}
// what the engine's path keeps beside the views (the fused state-transfer kernels: nothing)
static int setup_path(qoc_engine* e, const double* Hs, bool antiherm, const AutoPlan& plan) {
    const qoc_config& c = e->cfg;
    QocDev& d = e->d;
    std::string msg;
    int rc = QOC_OK;
    switch (e->path) {
    case QOC_PATH_MFMA:
        e->mf.variant = plan.latency ? 5 : c.variant;
        if (c.variant == 5 && !qoc_mfma_latency_ok(d))
            return fail(QOC_ERR_INVALID, "qoc_create: the latency mode of the MFMA path (variant 5) needs n <= 32 with k <= 8 (or, "
                "with at most 4 dressed forbidden levels, n <= 64), "
                                              "a Taylor degree >= 2 (n=%d k=%d T=%d)", c.n, c.k, d.T);
        // state transfer: sum_{j < T} A^j / j! is the polynomial of degree T - 1 (no squarings: d.s = 0)
        d.T = qoc_mfma_degree(d);
        rc = qoc_mfma_setup(e->mf, e->mp, d, c.chunks, (const cplx*)Hs, e->allocs, msg);
        if (rc) return fail(rc, "qoc_create: %s", msg.c_str());
        e->chunks = e->mf.C;
        break;
    case QOC_PATH_GEMM:
        if (c.time_shards >= 1) { e->gm.ts_G = c.time_shards; e->gm.ts_rank = c.time_rank; }
        e->gm.antiherm = antiherm;
        e->gm.direct_variant = c.path == QOC_PATH_GEMM ? c.variant : 0;
        rc = qoc_gemm_setup(e->gm, d, (const cplx*)Hs, plan.gemm_direct, e->allocs, msg);
        if (rc) return fail(rc, "qoc_create: %s", msg.c_str());
        if (!qoc_gemm_lds_opt_in()) return fail(QOC_ERR_HIP, "qoc_create: cannot reserve LDS for the GEMM-path kernels");
        e->chunks = e->gm.NC;
        if (e->gm.ts_G > 0) {
            std::string why;
            if (!qoc_gemm_ts_supported(e->gm, d, e->gm.ts_G, why))
                return fail(QOC_ERR_INVALID, "qoc_create: time_shards = %d needs %s (n=%d m=%d chunks=%d)", e->gm.ts_G, why.c_str(), c.n,
                    c.m, e->gm.NC);
            qoc_gemm_ts_ranges(e->gm, e->gm.ts_G);
        }
        break;
    case QOC_PATH_SMALL:
        rc = qoc_small_setup(e->sm, d, antiherm, c.chunks, c.variant, e->allocs, msg);
        if (rc) return fail(rc == -1 ? QOC_ERR_INVALID : (rc == -3 ? QOC_ERR_NOMEM : QOC_ERR_HIP),
            "qoc_create: %s (n=%d m=%d k=%d T=%d steps=%d seeds=%d)", msg.c_str(), c.n, c.m, c.k, d.T, c.steps, c.n_seeds);
        e->chunks = e->sm.G;
        [[fallthrough]];          // read-back (inter_vecs, final_state, unitary_scale) runs the any-size kernels on the last controls
    case QOC_PATH_GENERIC: return alloc_generic_scratch(e);
    }
    return QOC_OK;
}
static int setup_exact_gradient(qoc_engine* e) {
    const QocDev& d = e->d;
    if (const char* why = qoc_exact_plan(e->xg, d)) return fail(QOC_ERR_INVALID, "qoc_create: %s (T=%d s=%d)", why, d.T, d.s);
    TRY(dev_alloc(e, &e->xg.Lam, (size_t)d.B * d.steps * d.n * d.m));
    TRY(dev_alloc(e, &e->xg.scratch, (size_t)e->xg.grid * e->xg.per_wg));
    HIP_TRY_MSG(qoc_exact_lds_opt_in(e->xg), "qoc_create: cannot reserve %zu bytes of LDS for the exact gradient kernel", e->xg.lds_bytes);
    return QOC_OK;
}

// the group view of an ensemble engine: the caller's G control sets of k controls -- variable, Adam slots, stop rule, pulse regularisers,
// the tail's arrays -- beside the members' description and, for a pulse response, the response matrix
static int setup_group_view(qoc_engine* e, const EnsArgs& a) {
    const qoc_config& uc = *a.user;
    const qoc_ensemble& en = *a.ens;
    const int kg = uc.k, G = uc.n_seeds, E = en.members, q = en.n_perturb, steps = e->d.steps;
    QocDev& gv = e->g;
    gv = e->d;
    gv.k = kg; gv.B = G; gv.Bplan = G;
    // a pulse response: the group view is the SAMPLE view -- P samples of total_time / P each stand where the time slices stood, so the
    // pulse regularisers act on the samples with their coefficients divided by P
    if (a.shape) { gv.steps = a.shape->P; gv.dt = uc.total_time / (double)gv.steps; }
    fill_pulse_regularisers(gv, uc);
    // (the trajectories' buffers are not the groups'; omg and the bandpass arrays are null already: no trajectory has a pulse regulariser)
    gv.inter = nullptr; gv.Xfinal = nullptr; gv.ztau = nullptr; gv.Fpop = nullptr; gv.Fd = nullptr; gv.zfin = nullptr;
    gv.su_resid = nullptr;
    TRY(dev_upload(e, &gv.maxA, a.maxA, (size_t)kg));
    if (a.one_minus_gauss) TRY(dev_upload(e, &gv.omg, a.one_minus_gauss, (size_t)kg * gv.steps));
    TRY(alloc_set_arrays(e, gv, "qoc_create_ensemble", true));
    TRY(alloc_set_scalars(e, gv, "qoc_create_ensemble", "qoc_create_ensemble: the bandpass phase table could not be formed"));
    const double* da = nullptr; const double* dd = nullptr; const double* dw = nullptr;
    // the member tables: one block per device of a fleet, else one block that every control set reads
    const int F = a.fleet ? a.fleet->devices : 1;
    TRY(dev_upload(e, &da, a.fleet ? a.fleet->amp_scales : en.amp_scales, (size_t)F * E * kg));
    if (q > 0) TRY(dev_upload(e, &dd, a.fleet ? a.fleet->offsets : en.offsets, (size_t)F * E * q));
    TRY(dev_upload(e, &dw, en.weights, (size_t)E));
    e->en = QocEns{E, q, G / F, da, dd, dw};
    e->fleet_F = a.fleet ? F : 0;
    e->ens_wt.assign(en.weights, en.weights + E);
    if (const ShapeHost* shp = a.shape) {
        QocShape& sh = e->sh;
        sh.P = shp->P; sh.band = shp->band; sh.col_band = shp->col_band;
        TRY(dev_upload(e, &sh.Tt, shp->Tt.data(), (size_t)steps * shp->P));
        TRY(dev_upload(e, &sh.row_win, shp->row_win.data(), (size_t)steps));
        TRY(dev_upload(e, &sh.col_win, shp->col_win.data(), (size_t)shp->P));
        TRY(dev_alloc(e, &sh.uf, (size_t)G * kg * steps));
        e->shaped = true;
    }
    if (const qoc_control_map* cm = a.map) {
        // the pulse view and the map's arrays: the trajectories have r + q rows, the members' pulses k + q
        const int r = cm->n_terms, D = cm->degree;
        const size_t stage = (size_t)G * E * (kg + q) * steps;
        QocDev& pv = e->pv;
        pv = e->d;
        pv.k = kg + q;
        pv.u = nullptr; pv.dLdu = nullptr;
        TRY(dev_zalloc(e, &pv.u, stage, "qoc_create_mapped"));
        TRY(dev_zalloc(e, &pv.dLdu, stage, "qoc_create_mapped"));
        pv.w = pv.w2 = pv.u2 = pv.grad = pv.base = nullptr;
        e->cm = QocMap{r, D, kg, q, nullptr, nullptr, nullptr};
        TRY(dev_upload(e, &e->cm.alpha, cm->poly, (size_t)r * kg * D));
        if (cm->mix) TRY(dev_upload(e, &e->cm.M, cm->mix, (size_t)r * kg * steps));
        if (cm->fixed) TRY(dev_upload(e, &e->cm.F, cm->fixed, (size_t)r * steps));
        e->mapped = true;
    }
    return QOC_OK;
}

// the buffers of an open engine: collapse operators, the drift with -1/2 sum_j D_j^dagger D_j folded in, history, partials, populations
// (per member of an ensemble or fleet: a row of drifts with its rate scales s_j on D_j^dagger D_j, and the row of sqrt(s_j) that the kernels put on D_j)
static int setup_lindblad(qoc_engine* e, const Problem& p, const DecayHost* op) {
    const QocDev& d = e->d;
    QocLb& L = e->lb;
    const int n = d.n, c = op->c, rows = op->F * op->E;
    const size_t nn = (size_t)n * n, B = (size_t)d.B;
    L.on = 1; L.c = c; L.R = d.m * (d.m + 1) / 2; L.S = qoc_lb_stride(n); L.lds_bytes = qoc_lb_lds_bytes(n, c);
    L.E = op->E; L.Rs = d.B / rows; L.rows = rows;
    std::vector<double> dd(2 * nn * (size_t)c);                  // D_j^dagger D_j
    for (int j = 0; j < c; ++j) {
        const double* D = op->C + 2 * nn * (size_t)j;
        for (int a = 0; a < n; ++a)
            for (int b = 0; b < n; ++b) {
                double re = 0.0, im = 0.0;                       // (D^dagger D)[a][b] = sum_l conj(D[l][a]) D[l][b]
                for (int l = 0; l < n; ++l) {
                    const double xr = D[2 * (l * n + a)], xi = D[2 * (l * n + a) + 1], yr = D[2 * (l * n + b)], yi = D[2 * (l * n + b) + 1];
                    re += xr * yr + xi * yi;
                    im += xr * yi - xi * yr;
                }
                dd[2 * (nn * j + a * n + b)] = re; dd[2 * (nn * j + a * n + b) + 1] = im;
            }
    }
    std::vector<double> h0(2 * nn * (size_t)rows), rs;
    if (op->scales) rs.resize((size_t)rows * c);
    for (int row = 0; row < rows; ++row) {
        double* h = h0.data() + 2 * nn * (size_t)row;
        memcpy(h, p.Hs, 2 * nn * sizeof(double));
        for (int j = 0; j < c; ++j) {
            const double* x = dd.data() + 2 * nn * (size_t)j;
            // (no table: the plain -= 0.5 x of qoc_create_open, nothing scaled)
            if (!op->scales) { for (size_t i = 0; i < 2 * nn; ++i) h[i] -= 0.5 * x[i]; continue; }
            const double sc = op->scales[(size_t)row * c + j];
            rs[(size_t)row * c + j] = std::sqrt(sc);
            for (size_t i = 0; i < 2 * nn; ++i) h[i] -= 0.5 * (sc * x[i]);
        }
    }
    TRY(dev_upload(e, &L.H0, (const cplx*)h0.data(), nn * rows));
    if (c > 0) TRY(dev_upload(e, &L.D, (const cplx*)op->C, (size_t)c * nn));
    if (c > 0 && op->scales) TRY(dev_upload(e, &L.rs, (const double*)rs.data(), rs.size()));
    TRY(dev_alloc(e, &L.hist, B * L.R * d.steps * nn));
    TRY(dev_alloc(e, &L.partial, B * L.R * d.k * d.steps));
    TRY(dev_alloc(e, &L.pop, B * (d.steps + 1) * n * d.m));
    if (op->costs) {
        // running costs: the observables as they came, the coefficients divided by steps (as every state regulariser's are)
        const int nc = op->costs->n_obs;
        std::vector<double> ca(op->costs->coeffs, op->costs->coeffs + nc);
        for (double& a : ca) a /= (double)d.steps;
        L.nc = nc;
        TRY(dev_upload(e, &L.cO, (const cplx*)op->costs->O, nn * nc));
        TRY(dev_upload(e, &L.ca, (const double*)ca.data(), (size_t)nc));
        TRY(dev_upload(e, &L.cp, (const int*)op->costs->powers, (size_t)nc));
        TRY(dev_alloc(e, &L.cost_partial, B * L.R));
        TRY(dev_alloc(e, &L.expct, B * (d.steps + 1) * nc * d.m));
    }
    if (e->path == QOC_PATH_LINDBLAD_TILED) {
        // the tiled kernels: no LDS to reserve; the table of D_j padded to NP x NP and scaled per row (lb_setup's product), the workgroups' scratch
        QocLbt& W = e->lbt;
        const int NP = qoc_lbt_np(n);
        const size_t mat = (size_t)NP * NP;
        W.on = 1; W.NP = NP; W.work_bytes = B * L.R * QOC_LBT_MATS * mat * sizeof(cplx);
        L.S = NP; L.lds_bytes = 0;
        if (c > 0) {
            std::vector<double> dp(2 * mat * (size_t)c * rows, 0.0);
            for (int row = 0; row < rows; ++row)
                for (int j = 0; j < c; ++j) {
                    const double sc = op->scales ? rs[(size_t)row * c + j] : 1.0;
                    const double* D = op->C + 2 * nn * (size_t)j;
                    double* o = dp.data() + 2 * mat * ((size_t)row * c + j);
                    for (int a = 0; a < n; ++a)
                        for (int b = 0; b < n; ++b) {
                            // (no table: D_j as it came, nothing scaled)
                            o[2 * ((size_t)a * NP + b)] = op->scales ? D[2 * (a * n + b)] * sc : D[2 * (a * n + b)];
                            o[2 * ((size_t)a * NP + b) + 1] = op->scales ? D[2 * (a * n + b) + 1] * sc : D[2 * (a * n + b) + 1];
                        }
                }
            TRY(dev_upload(e, &W.Dp, (const cplx*)dp.data(), mat * c * rows));
        }
        TRY(dev_alloc(e, &W.work, B * L.R * QOC_LBT_MATS * mat));
        return QOC_OK;
    }
    HIP_TRY_MSG(qoc_lb_lds_opt_in(L), "%s: cannot reserve %zu bytes of LDS for the open-system kernels", op->who, L.lds_bytes);
    return QOC_OK;
}

// the buffers of a sparse engine: the ELLPACK blocks in one pool, the costates of every slice, the vectors' scratch when they do not live in LDS
static int setup_sparse(qoc_engine* e, const SparseHost& h) {
    const QocDev& d = e->d;
    QocSparse& sp = e->sp;
    // QOC_EXPERIMENTAL=1 QOC_SP_THREADS=256|1024: the sweeps' workgroup size, for the A/B runs behind QOC_SP_WIDE_FROM
    int threads = 0;
    if (const char* t = qoc_exp_env("QOC_SP_THREADS")) threads = atoi(t) == 1024 ? 1024 : (atoi(t) == 256 ? 256 : 0);
    if (const char* why = qoc_sp_plan(sp, d, h.vector_home, threads, h.merged, (int)h.ops.size())) return fail(QOC_ERR_INVALID, "%s: %s (n = %d)", h.who, why, d.n);
    const size_t n = (size_t)d.n, K = h.ops.size();
    e->sp_fleet_entry = h.fleet_entry;
    if (h.kgrad >= 0 && h.kgrad < d.k) {
        // the frozen perturbation rows of the trajectories' gradient: cleared once, never written (k_sp_grad stops at kgrad) and never read
        sp.kgrad = h.kgrad;
        HIP_TRY(hipMemset(d.dLdu, 0, (size_t)d.B * d.k * d.steps * sizeof(double)));
    }
    if (h.merged) {
        // the merged rows beside the per-operator blocks (which k_sp_grad keeps reading)
        const size_t slots = n * (size_t)h.rows.Wm;
        sp.Wm = h.rows.Wm;
        TRY(dev_upload(e, &sp.mlen, (const int*)h.rows.len.data(), n));
        if (slots) {
            TRY(dev_upload(e, &sp.midx, (const int*)h.rows.idx.data(), slots));
            TRY(dev_upload(e, &sp.mval, (const cplx*)h.rows.val.data(), slots));
        }
    }
    std::vector<int> W(K);
    std::vector<long long> off(K);
    size_t total = 0;
    for (size_t j = 0; j < K; ++j) { W[j] = h.ops[j].W; off[j] = (long long)total; total += n * (size_t)W[j]; sp.stored += h.ops[j].stored; }
    int* col = nullptr;
    cplx* val = nullptr;
    TRY(dev_alloc(e, &col, total));
    TRY(dev_alloc(e, &val, total));
    for (size_t j = 0; j < K; ++j) {
        if (!W[j]) continue;
        HIP_TRY(hipMemcpy(col + off[j], h.ops[j].col.data(), n * W[j] * sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(val + off[j], h.ops[j].val.data(), n * W[j] * sizeof(cplx), hipMemcpyHostToDevice));
    }
    sp.col = col; sp.val = val;
    e->sp_widths = W;
    TRY(dev_upload(e, &sp.W, (const int*)W.data(), K));
    TRY(dev_upload(e, &sp.off, (const long long*)off.data(), K));
    TRY(dev_alloc(e, &sp.Lam, (size_t)d.B * d.steps * n * d.m));
    if (sp.home == 2) TRY(dev_alloc(e, &sp.scratch, (size_t)d.B * d.m * 2 * n));
    HIP_TRY_MSG(qoc_sp_lds_opt_in(sp), "%s: cannot reserve %zu bytes of LDS for the sparse sweeps", h.who, sp.lds_bytes);
    return QOC_OK;
}

static int create_engine(const qoc_config* cfg, const Problem& p, const EnsArgs* ens, qoc_handle* out) {
    const DecayHost* open = p.decay;
    TRY(check_create_args(cfg, p, out));
    HIP_TRY(hipSetDevice(cfg->device));
    // the half-built engine owns itself: every early return below destroys it (fail() has set the message by then)
    std::unique_ptr<qoc_engine, int (*)(qoc_handle)> guard(new qoc_engine(), qoc_destroy);
    qoc_engine* e = guard.get();
    e->cfg = *cfg;
    if (ens) e->ens_E = ens->ens->members;
    // the trajectory view: the shape, the state regularisers and (a plain engine: its control sets are the trajectories) the pulse's
    QocDev& d = e->d;
    memset(&d, 0, sizeof d);
    d.n = cfg->n; d.k = cfg->k; d.steps = cfg->steps; d.m = cfg->m; d.T = cfg->taylor_terms; d.s = cfg->state_transfer ? 0 : cfg->scaling;
    d.B = cfg->n_seeds; d.state_transfer = cfg->state_transfer; d.dt = cfg->dt;
    if (open) d.s = cfg->scaling;                                // (an open engine takes sub-steps in both modes)
    d.Bplan = cfg->plan_seeds > 0 ? cfg->plan_seeds : cfg->n_seeds;
    fill_pulse_regularisers(d, *cfg);
    d.has_speed = cfg->has_speed_up; d.a_speed = cfg->c_speed_up * (1.0 / (double)cfg->steps);
    d.n_forb = cfg->n_forbidden; d.forbid_dressed = cfg->forbid_dressed && cfg->n_forbidden > 0;
    HIP_TRY_MSG(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking), "hipStreamCreate failed");
    HIP_TRY_MSG(hipEventCreate(&e->t0), "hipEventCreate failed");
    HIP_TRY_MSG(hipEventCreate(&e->t1), "hipEventCreate failed");
    TRY(build_trajectory_view(e, p));
    const bool antiherm = p.sparse ? false : cfg->state_transfer ? qoc_all_antihermitian((const cplx*)p.Hs, cfg->n, cfg->k + 1) : true;
    AutoPlan plan{};
    // (an open engine has been through build_trajectory_view like every engine: d.inter, d.Xfinal, d.ztau and zfin are allocated there and never
    // touched by the open path -- (steps + 1) n m + n^2 numbers per control set, small beside its history; left so as not to fork that helper)
    // (AUTO is the LDS path, as it was: no table to consult, and no crossover measured; the tiled path is taken by name)
    if (open) plan.path = cfg->path == QOC_PATH_LINDBLAD_TILED ? QOC_PATH_LINDBLAD_TILED : QOC_PATH_LINDBLAD;
    else if (p.sparse) plan.path = QOC_PATH_SPARSE;
    else TRY(choose_path(*cfg, d, antiherm, ens != nullptr, plan));
    e->path = plan.path; e->chunks = 1;
#ifdef QOC_DEBUG     // timing experiments only (tools/skip_timing.py builds its own library with -DQOC_DEBUG): never in the product library
    if (const char* sk = getenv("QOC_DEBUG_SKIP")) {             // wall-clock attribution of one kernel group
        e->skip_mask = atoi(sk);
        if (e->skip_mask) fprintf(stderr, "libqoc_hip: WARNING: QOC_DEBUG_SKIP=%d is set -- kernel groups are skipped or repeated, every "
            "result of this engine is garbage (timing experiments only)\n", e->skip_mask);
    }
#endif
    if (open) TRY(setup_lindblad(e, p, open));
    else if (p.sparse) TRY(setup_sparse(e, *p.sparse));
    else TRY(setup_path(e, p.Hs, antiherm, plan));
    if (cfg->gradient == 1) TRY(setup_exact_gradient(e));
    if (ens) TRY(setup_group_view(e, *ens));
    const hipError_t se = hipDeviceSynchronize();
    HIP_TRY_MSG(se, "qoc_create: %s", hipGetErrorString(se));
    *out = guard.release();
    return QOC_OK;
}

extern "C" {

const char* qoc_last_error(void) { return g_err.c_str(); }
const char* qoc_version(void) { return "qoc-hip 0.1 (gfx950)"; }

int qoc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int qoc_device_info(int32_t device, char* name, int32_t name_len, int32_t* compute_units, int64_t* hbm_bytes) {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (name && name_len > 0) {
        snprintf(name, (size_t)name_len, "%s (%s)", prop.name, prop.gcnArchName);
    }
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    return QOC_OK;
}

int qoc_device_peer_access(int32_t device, int32_t peer, int32_t* can_access) {
    if (!can_access) return fail(QOC_ERR_INVALID, "qoc_device_peer_access: null argument");
    int can = 0;
    if (device == peer) can = 1;
    else HIP_TRY(hipDeviceCanAccessPeer(&can, device, peer));
    *can_access = can;
    return QOC_OK;
}

int qoc_create(const qoc_config* cfg, const double* Hs, const double* U0, const double* V, const double* W,
               const double* maxA, const double* one_minus_gauss, const int32_t* forbidden_states,
               const double* forbidden_coeffs, const double* Vs, qoc_handle* out) {
    return create_engine(cfg, Problem{Hs, U0, V, W, maxA, one_minus_gauss, forbidden_states, forbidden_coeffs, Vs}, nullptr, out);
}

// what an open engine refuses, on the host and before any device is touched (`who`: qoc_create_open or qoc_create_open_fleet)
static int check_open(const char* who, const qoc_config* cfg, int c, const double* C) {
    const int n = cfg->n;
    if (cfg->n_forbidden > 0) return fail(QOC_ERR_INVALID, "%s: forbidden levels are not available under a master equation (n_forbidden = %d)", who, cfg->n_forbidden);
    if (cfg->has_speed_up) return fail(QOC_ERR_INVALID, "%s: the speed_up regulariser is not available under a master equation", who);
    if (cfg->forbid_dressed) return fail(QOC_ERR_INVALID, "%s: forbid_dressed is not available under a master equation", who);
    if (cfg->gradient != 0) return fail(QOC_ERR_INVALID, "%s: the exact gradient is not available under a master equation (gradient = %d)", who, cfg->gradient);
    if (cfg->time_shards > 0) return fail(QOC_ERR_INVALID, "%s: an open system cannot be time-sharded (time_shards = %d)", who, cfg->time_shards);
    const bool tiled = cfg->path == QOC_PATH_LINDBLAD_TILED;     // (taken by name only: 1 .. 128 levels, no LDS rule)
    if (cfg->path != QOC_PATH_AUTO && cfg->path != QOC_PATH_LINDBLAD && !tiled)
        return fail(QOC_ERR_INVALID, "%s: an open system runs on QOC_PATH_LINDBLAD (or AUTO), not on path %d", who, cfg->path);
    if (c < 0 || (c > 0 && !C)) return fail(QOC_ERR_INVALID, "%s: n_collapse = %d (>= 0) with its operators", who, c);
    if (tiled && (n < 1 || n > QOC_LBT_MAX_N))
        return fail(QOC_ERR_INVALID, "%s: n = %d (1 .. %d levels on QOC_PATH_LINDBLAD_TILED)", who, n, QOC_LBT_MAX_N);
    if (!tiled && (n < 1 || n > QOC_LB_MAX_N)) return fail(QOC_ERR_INVALID, "%s: n = %d (1 .. %d levels)", who, n, QOC_LB_MAX_N);
    if (c > QOC_LB_MAX_C) return fail(QOC_ERR_INVALID, "%s: n_collapse = %d (at most %d collapse operators)", who, c, QOC_LB_MAX_C);
    if (cfg->m < 1 || cfg->m > n) return fail(QOC_ERR_INVALID, "%s: m = %d states of interest (1 .. n = %d)", who, cfg->m, n);
    if (!tiled && qoc_lb_lds_bytes(n, c) > QOC_LB_LDS_LIMIT)
        return fail(QOC_ERR_INVALID, "%s: n = %d with %d collapse operators needs %zu bytes of LDS (limit %zu)", who, n, c, qoc_lb_lds_bytes(n, c),
                    QOC_LB_LDS_LIMIT);
    if (cfg->taylor_terms < 1 || cfg->taylor_terms > QOC_LB_MAX_T)
        return fail(QOC_ERR_INVALID, "%s: taylor_terms = %d (1 .. %d)", who, cfg->taylor_terms, QOC_LB_MAX_T);
    if (cfg->scaling < 0 || cfg->scaling > QOC_LB_MAX_S) return fail(QOC_ERR_INVALID, "%s: scaling = %d (0 .. %d)", who, cfg->scaling, QOC_LB_MAX_S);
    for (size_t i = 0; i < 2 * (size_t)c * n * n; ++i)
        if (!std::isfinite(C[i])) return fail(QOC_ERR_INVALID, "%s: a collapse operator is not finite", who);
    return QOC_OK;
}

int qoc_create_open(const qoc_config* cfg, const qoc_open* open, const double* Hs, const double* U0, const double* V, const double* W,
                    const double* maxA, const double* one_minus_gauss, qoc_handle* out) {
    if (!cfg || !open || !Hs || !V || !W || !maxA || !out) return fail(QOC_ERR_INVALID, "qoc_create_open: null argument");
    TRY(check_open("qoc_create_open", cfg, open->n_collapse, open->C));
    const DecayHost dh{open->n_collapse, open->C, nullptr, 1, 1, "qoc_create_open"};
    return create_engine(cfg, Problem{Hs, U0, V, W, maxA, one_minus_gauss, nullptr, nullptr, nullptr, nullptr, &dh}, nullptr, out);
}

// what a sparse engine refuses about its configuration and its operators (K of them), on the host and before any device is touched; then COO ->
// ELLPACK: indices in range, values finite, n W_j within int32 (`who`: qoc_create_sparse or qoc_create_sparse_fleet)
static int check_sparse(const char* who, const qoc_config* cfg, const qoc_sparse* ops, int K, SparseHost& sh) {
    if (!cfg->state_transfer) return fail(QOC_ERR_INVALID, "%s: sparse operators run in state-transfer mode only (unitary mode propagates an n x n matrix)", who);
    if (cfg->forbid_dressed) return fail(QOC_ERR_INVALID, "%s: forbid_dressed needs the n x n matrix of dressed states; forbidden levels are bare on a sparse engine", who);
    if (cfg->gradient != 0) return fail(QOC_ERR_INVALID, "%s: the exact gradient is not available on sparse operators (gradient = %d)", who, cfg->gradient);
    if (cfg->time_shards > 0) return fail(QOC_ERR_INVALID, "%s: a sparse engine cannot be time-sharded (time_shards = %d)", who, cfg->time_shards);
    if (cfg->path != QOC_PATH_AUTO && cfg->path != QOC_PATH_SPARSE)
        return fail(QOC_ERR_INVALID, "%s: sparse operators run on QOC_PATH_SPARSE (or AUTO), not on path %d", who, cfg->path);
    if (cfg->n < 1 || cfg->k < 1 || cfg->steps < 1 || cfg->n_seeds < 1) return fail(QOC_ERR_INVALID, "%s: n, k, steps, n_seeds must be >= 1", who);
    if (cfg->taylor_terms < 1 || cfg->taylor_terms > QOC_SP_MAX_T)
        return fail(QOC_ERR_INVALID, "%s: taylor_terms = %d (1 .. %d)", who, cfg->taylor_terms, QOC_SP_MAX_T);
    if (cfg->m < 1) return fail(QOC_ERR_INVALID, "%s: m = %d states of interest (>= 1)", who, cfg->m);
    if ((long long)cfg->n * cfg->m > (long long)INT32_MAX) return fail(QOC_ERR_INVALID, "%s: n * m = %d * %d does not fit 32-bit indices", who, cfg->n, cfg->m);
    if (ops->vector_home < 0 || ops->vector_home > 2) return fail(QOC_ERR_INVALID, "%s: vector_home = %d (0 auto, 1 LDS, 2 global scratch)", who, ops->vector_home);
    if (ops->vector_home == 1 && 2 * (size_t)cfg->n * sizeof(cplx) > QOC_SP_LDS_LIMIT)
        return fail(QOC_ERR_INVALID, "%s: vector_home = 1 (LDS) needs 2 n 16 bytes <= 159 KiB (n = %d, at most 5088)", who, cfg->n);
    if (!ops->indptr) return fail(QOC_ERR_INVALID, "%s: indptr is missing", who);
    for (int j = 0; j < K; ++j)
        if (ops->indptr[j] < 0 || ops->indptr[j + 1] < ops->indptr[j]) return fail(QOC_ERR_INVALID, "%s: indptr[%d .. %d] does not ascend from 0", who, j, j + 1);
    if (ops->indptr[K] > 0 && (!ops->row || !ops->col || !ops->val)) return fail(QOC_ERR_INVALID, "%s: entry arrays missing", who);
    sh.who = who;
    sh.vector_home = ops->vector_home;
    sh.ops.resize((size_t)K);
    std::string why;
    for (int j = 0; j < K; ++j) {
        const int64_t a = ops->indptr[j], cnt = ops->indptr[j + 1] - a;
        if (!qoc_ell_build(cfg->n, cnt, ops->row + a, ops->col + a, ops->val + 2 * a, sh.ops[(size_t)j], why))
            return fail(QOC_ERR_INVALID, "%s: operator %d: %s", who, j, why.c_str());
    }
    return QOC_OK;
}

int qoc_create_sparse(const qoc_config* cfg, const qoc_sparse* ops, const double* V, const double* W, const double* maxA,
                      const double* one_minus_gauss, const int32_t* forbidden_states, const double* forbidden_coeffs, qoc_handle* out) {
    if (!cfg || !ops || !V || !W || !maxA || !out) return fail(QOC_ERR_INVALID, "qoc_create_sparse: null argument");
    SparseHost sh;
    TRY(check_sparse("qoc_create_sparse", cfg, ops, cfg->k + 1, sh));
    return create_engine(cfg, Problem{nullptr, nullptr, V, W, maxA, one_minus_gauss, forbidden_states, forbidden_coeffs, nullptr, &sh}, nullptr, out);
}

// the map of qoc_create_mapped and of every entry point that takes one (`who`), checked on the host and before any device is touched: ranges,
// finite entries, every pulse reaches an operator
static int check_map(const char* who, const qoc_config* cfg, const qoc_control_map* map, const double* maxA) {
    if (!cfg || !maxA) return fail(QOC_ERR_INVALID, "%s: null argument", who);
    if (!map) return fail(QOC_ERR_INVALID, "%s: the control map is missing", who);
    if (!map->poly) return fail(QOC_ERR_INVALID, "%s: the map's polynomial coefficients (poly) are missing", who);
    if (cfg->k < 1 || cfg->steps < 1) return fail(QOC_ERR_INVALID, "%s: k, steps must be >= 1", who);
    const int r = map->n_terms, D = map->degree, k = cfg->k, steps = cfg->steps;
    if (r < 1 || r > QOC_MAP_MAX_TERMS) return fail(QOC_ERR_INVALID, "%s: n_terms = %d (1 .. %d operators)", who, r, QOC_MAP_MAX_TERMS);
    if (D < 1 || D > QOC_MAP_MAX_DEGREE) return fail(QOC_ERR_INVALID, "%s: degree = %d (1 .. %d)", who, D, QOC_MAP_MAX_DEGREE);
    for (size_t i = 0; i < (size_t)r * k * D; ++i)
        if (!std::isfinite(map->poly[i])) return fail(QOC_ERR_INVALID, "%s: poly[%zu][%zu][%zu] is not finite", who, i / ((size_t)k * D), (i / D) % k, i % D);
    if (map->mix)
        for (size_t i = 0; i < (size_t)r * k * steps; ++i)
            if (!std::isfinite(map->mix[i]))
                return fail(QOC_ERR_INVALID, "%s: mix[%zu][%zu][%zu] is not finite", who, i / ((size_t)k * steps), (i / steps) % k, i % steps);
    if (map->fixed)
        for (size_t i = 0; i < (size_t)r * steps; ++i)
            if (!std::isfinite(map->fixed[i])) return fail(QOC_ERR_INVALID, "%s: fixed[%zu][%zu] is not finite", who, i / steps, i % steps);
    for (int j = 0; j < k; ++j) {
        bool reaches = false;
        for (int i = 0; i < r && !reaches; ++i) {
            bool poly = false, mix = !map->mix;
            for (int d = 0; d < D; ++d) poly = poly || map->poly[((size_t)i * k + j) * D + d] != 0.0;
            for (int t = 0; t < steps && !mix; ++t) mix = map->mix[((size_t)i * k + j) * steps + t] != 0.0;
            reaches = poly && mix;
        }
        if (!reaches) return fail(QOC_ERR_INVALID, "%s: pulse %d reaches no operator (poly[i][%d] or mix[i][%d] is zero for every i)", who, j, j, j);
    }
    return QOC_OK;
}

// the fleet's own checks (`who`), on the host and before any device is touched: its tables are read in place of the ensemble's offsets and
// amp_scales, E members with q perturbations on each of its devices
static int check_fleet(const char* who, const qoc_config* cfg, const qoc_fleet* fleet, const double* maxA, int E, int q) {
    if (!cfg || !maxA) return fail(QOC_ERR_INVALID, "%s: null argument", who);
    if (!fleet) return fail(QOC_ERR_INVALID, "%s: the fleet is missing", who);
    if (!fleet->amp_scales) return fail(QOC_ERR_INVALID, "%s: the fleet's amp_scales are missing", who);
    if (cfg->k < 1 || cfg->n_seeds < 1) return fail(QOC_ERR_INVALID, "%s: k, n_seeds must be >= 1", who);
    const int F = fleet->devices, k = cfg->k;
    if (F < 1) return fail(QOC_ERR_INVALID, "%s: devices = %d (>= 1)", who, F);
    if (cfg->n_seeds % F != 0) return fail(QOC_ERR_INVALID, "%s: n_seeds = %d is no multiple of devices = %d", who, cfg->n_seeds, F);
    if (E < 1 || q < 0) return fail(QOC_ERR_INVALID, "%s: members = %d (>= 1), n_perturb = %d (>= 0)", who, E, q);
    if (q > 0 && !fleet->offsets) return fail(QOC_ERR_INVALID, "%s: the fleet's offsets are missing (n_perturb = %d)", who, q);
    const size_t per_a = (size_t)E * k, per_d = (size_t)E * q;
    for (size_t i = 0; i < (size_t)F * per_a; ++i)
        if (!std::isfinite(fleet->amp_scales[i]))
            return fail(QOC_ERR_INVALID, "%s: amp_scales[%zu][%zu][%zu] is not finite", who, i / per_a, (i / k) % E, i % k);
    for (size_t i = 0; i < (size_t)F * per_d; ++i)
        if (!std::isfinite(fleet->offsets[i]))
            return fail(QOC_ERR_INVALID, "%s: offsets[%zu][%zu][%zu] is not finite", who, i / per_d, (i / q) % E, i % q);
    return QOC_OK;
}

// the response matrix of a line (`who`), checked on the host: finite, every sample reaches the pulse; then the nonzero window of every row and
// column and the transposed copy
static int build_shape(const char* who, const qoc_config* cfg, const qoc_transfer* tr, ShapeHost& sh) {
    if (cfg->k < 1 || cfg->steps < 1) return fail(QOC_ERR_INVALID, "%s: k, steps must be >= 1", who);
    const int steps = cfg->steps, P = tr->n_samples;
    if (P < 1) return fail(QOC_ERR_INVALID, "%s: n_samples = %d (>= 1)", who, P);
    if (!tr->T) return fail(QOC_ERR_INVALID, "%s: the response matrix is missing", who);
    if (cfg->has_envelope) return fail(QOC_ERR_INVALID, "%s: the envelope regulariser is defined per time slice, not per sample", who);
    sh = ShapeHost{P, 0, 0, std::vector<double>((size_t)P * steps), std::vector<int2>((size_t)steps, make_int2(0, 0)),
                   std::vector<int2>((size_t)P, make_int2(0, 0))};
    for (int t = 0; t < steps; ++t)
        for (int s = 0; s < P; ++s) {
            const double v = tr->T[(size_t)t * P + s];
            if (!std::isfinite(v)) return fail(QOC_ERR_INVALID, "%s: T[%d][%d] is not finite", who, t, s);
            sh.Tt[(size_t)s * steps + t] = v;
            if (v != 0.0) {
                int2& r = sh.row_win[t];
                int2& c = sh.col_win[s];
                if (r.x == r.y) r.x = s;
                r.y = s + 1;
                if (c.x == c.y) c.x = t;
                c.y = t + 1;
            }
        }
    for (int s = 0; s < P; ++s) {
        if (sh.col_win[s].x == sh.col_win[s].y) return fail(QOC_ERR_INVALID, "%s: column %d of T is zero (the sample never reaches the pulse)", who, s);
        sh.col_band = std::max(sh.col_band, sh.col_win[s].y - sh.col_win[s].x);
    }
    for (int t = 0; t < steps; ++t) sh.band = std::max(sh.band, sh.row_win[t].y - sh.row_win[t].x);
    return QOC_OK;
}

// what an entry point composes its engine from, each null where it has none: the ensemble (null: one nominal member), the fleet's member tables,
// the line's response matrix, the control map
struct Glue { const qoc_ensemble* ens; const qoc_fleet* fleet; const qoc_transfer* tr; const qoc_control_map* map; };

// The one way from every entry point but qoc_create to create_engine (`who` names the entry point in the messages).  An entry point has run its
// own checks by now -- the glue it requires, check_open and the running costs, check_sparse and the row layout -- and filled p, decay and sparse
// included.  What follows is checked in this order, on the host and before any device is touched, and the first defect names the refusal:
//   1. cfg and maxA present                                                          "<who>: null argument"
//   2. the fleet, when there is one (check_fleet): presence, amp_scales, k / n_seeds, devices, divisibility, members / n_perturb, offsets
//      present, both tables finite
//   3. the control map, when there is one (check_map)
//   4. the response matrix, when there is one (build_shape): n_samples, T present, no envelope, finite, no zero column
//   5. the members: Hs and out present, members / n_perturb, the ensemble's arrays, the sizes, weights, rate scales, what an ensemble cannot
//      run on (time shards, QOC_PATH_SMALL, the latency mode, the 8-control paths); then the trajectory configuration
//   6. create_engine (check_create_args speaks as qoc_create)
static int create_composed(const char* who, const qoc_config* cfg, const Glue& g, Problem p, qoc_handle* out) {
    if (!cfg || !p.maxA) return fail(QOC_ERR_INVALID, "%s: null argument", who);
    // no ensemble: one nominal member; on a fleet the members' offsets and amp_scales are the fleet's and the ensemble's own are not read
    const std::vector<double> ones((size_t)std::max(cfg->k, 0) + 1, 1.0);
    qoc_ensemble members = g.ens ? *g.ens : qoc_ensemble{1, 0, nullptr, nullptr, ones.data(), ones.data()};
    const qoc_ensemble* ens = &members;
    const qoc_fleet* fleet = g.fleet;
    const qoc_control_map* map = g.map;
    if (fleet) {
        TRY(check_fleet(who, cfg, fleet, p.maxA, members.members, members.n_perturb));
        members.offsets = nullptr; members.amp_scales = nullptr;
    }
    if (map) TRY(check_map(who, cfg, map, p.maxA));
    ShapeHost shape;
    if (g.tr) TRY(build_shape(who, cfg, g.tr, shape));
    if ((!p.Hs && !p.sparse) || !out) return fail(QOC_ERR_INVALID, "%s: null argument", who);
    const int E = ens->members, q = ens->n_perturb;
    if (E < 1 || q < 0) return fail(QOC_ERR_INVALID, "%s: members = %d (>= 1), n_perturb = %d (>= 0)", who, E, q);
    if ((!fleet && !ens->amp_scales) || !ens->weights || (q > 0 && ((!ens->P && !p.sparse) || (!fleet && !ens->offsets))))
        return fail(QOC_ERR_INVALID, "%s: ensemble arrays missing", who);
    if (cfg->n < 1 || cfg->k < 1 || cfg->steps < 1 || cfg->n_seeds < 1 || cfg->plan_seeds < 0)
        return fail(QOC_ERR_INVALID, "%s: n, k, steps, n_seeds must be >= 1", who);
    if ((long long)cfg->n_seeds * E > (1 << 24)) return fail(QOC_ERR_INVALID, "%s: %d x %d trajectories", who, cfg->n_seeds, E);
    if (cfg->has_envelope && !p.one_minus_gauss) return fail(QOC_ERR_INVALID, "%s: envelope constant missing", who);
    if (cfg->has_d2wdt2 && !cfg->has_dwdt) return fail(QOC_ERR_INVALID, "%s: d2wdt2 needs dwdt (reference: NameError new_weights)", who);
    for (int i = 0; i < E; ++i)
        if (!(ens->weights[i] >= 0.0)) return fail(QOC_ERR_INVALID, "%s: weight %d is %g", who, i, ens->weights[i]);
    // (an open engine: the members' rate scales, a row of c for each of the F E members just checked)
    if (p.decay && p.decay->scales) {
        const size_t c = (size_t)p.decay->c, rows = (size_t)(fleet ? fleet->devices : 1) * E;
        for (size_t i = 0; i < rows * c; ++i) {
            const double v = p.decay->scales[i];
            if (!std::isfinite(v) || v < 0.0)
                return fail(QOC_ERR_INVALID, "%s: rate_scales[%zu][%zu][%zu] is %g (finite, >= 0)", who, i / ((size_t)E * c), (i / c) % E, i % c, v);
        }
    }
    // paths whose tail runs inside their own launch, or that form their controls from the variable, cannot host the member reduction
    if (cfg->time_shards > 0) return fail(QOC_ERR_INVALID, "%s: an ensemble cannot be time-sharded (time_shards = %d)", who, cfg->time_shards);
    if (cfg->path == QOC_PATH_SMALL) return fail(QOC_ERR_INVALID, "%s: the workgroup-resident path (QOC_PATH_SMALL) runs its tail "
        "inside its launch, where the members' gradients cannot be reduced first", who);
    if (!p.decay && cfg->variant == 5 && (cfg->path == QOC_PATH_AUTO || cfg->path == QOC_PATH_MFMA)) return fail(QOC_ERR_INVALID,
        "%s: the latency mode of the MFMA path (variant 5) forms its controls from the variable and fuses its tail", who);
    // (a control map: the trajectories run the r operators the map feeds)
    const int kt = map ? map->n_terms : cfg->k;
    if ((cfg->path == QOC_PATH_MFMA || cfg->path == QOC_PATH_ST_FUSED) && kt + q > 8) return fail(QOC_ERR_INVALID,
        "%s: path %d is limited to 8 controls; the ensemble's trajectories have %s + q = %d", who, cfg->path, map ? "r" : "k", kt + q);
    // the trajectories: G E of them, k + q controls (the perturbations are frozen control rows), no pulse regulariser (the group view has them)
    qoc_config tc = *cfg;
    const int n = cfg->n, k = cfg->k;
    const size_t nn = (size_t)n * n;
    tc.k = kt + q;
    tc.n_seeds = cfg->n_seeds * E;
    tc.plan_seeds = cfg->plan_seeds > 0 ? cfg->plan_seeds * E : 0;
    tc.has_amplitude = tc.has_envelope = tc.has_dwdt = tc.has_d2wdt2 = tc.has_bandpass = 0;
    tc.c_amplitude = tc.c_envelope = tc.c_dwdt = tc.c_d2wdt2 = tc.c_bandpass = 0.0;
    // (sparse operators: the SparseHost carries the kt + q + 1 ELLPACK blocks already; no dense array is stacked)
    std::vector<double> Hst(p.sparse ? 0 : 2 * nn * (size_t)(kt + q + 1));
    if (!p.sparse) memcpy(Hst.data(), p.Hs, 2 * nn * (size_t)(kt + 1) * sizeof(double));
    if (!p.sparse && q > 0) memcpy(Hst.data() + 2 * nn * (size_t)(kt + 1), ens->P, 2 * nn * (size_t)q * sizeof(double));
    // (no trajectory kernel of an ensemble forms controls from maxA: the rows of a mapped engine carry ones)
    std::vector<double> maxAt(p.maxA, p.maxA + (map ? 0 : k));
    maxAt.resize((size_t)(kt + q), 1.0);
    const EnsArgs ea{cfg, p.maxA, cfg->has_envelope ? p.one_minus_gauss : nullptr, ens, g.tr ? &shape : nullptr, map, fleet};
    p.Hs = p.sparse ? nullptr : Hst.data(); p.maxA = maxAt.data(); p.one_minus_gauss = nullptr;
    return create_engine(&tc, p, &ea, out);
}

int qoc_create_ensemble(const qoc_config* cfg, const qoc_ensemble* ens, const double* Hs, const double* U0, const double* V, const double* W,
                        const double* maxA, const double* one_minus_gauss, const int32_t* forbidden_states,
                        const double* forbidden_coeffs, const double* Vs, qoc_handle* out) {
    if (!ens) return fail(QOC_ERR_INVALID, "qoc_create_ensemble: null argument");
    return create_composed("qoc_create_ensemble", cfg, Glue{ens, nullptr, nullptr, nullptr},
                           Problem{Hs, U0, V, W, maxA, one_minus_gauss, forbidden_states, forbidden_coeffs, Vs}, out);
}

int qoc_create_shaped(const qoc_config* cfg, const qoc_ensemble* ens, const qoc_transfer* tr, const double* Hs, const double* U0, const double* V,
                      const double* W, const double* maxA, const double* one_minus_gauss, const int32_t* forbidden_states,
                      const double* forbidden_coeffs, const double* Vs, qoc_handle* out) {
    if (!tr) return fail(QOC_ERR_INVALID, "qoc_create_shaped: null argument");
    return create_composed("qoc_create_shaped", cfg, Glue{ens, nullptr, tr, nullptr},
                           Problem{Hs, U0, V, W, maxA, one_minus_gauss, forbidden_states, forbidden_coeffs, Vs}, out);
}

int qoc_create_mapped(const qoc_config* cfg, const qoc_ensemble* ens, const qoc_transfer* tr, const qoc_control_map* map, const double* Hs,
                      const double* U0, const double* V, const double* W, const double* maxA, const double* one_minus_gauss,
                      const int32_t* forbidden_states, const double* forbidden_coeffs, const double* Vs, qoc_handle* out) {
    if (!map) return check_map("qoc_create_mapped", cfg, map, maxA);           // (refused there: a null argument, or the map named as missing)
    return create_composed("qoc_create_mapped", cfg, Glue{ens, nullptr, tr, map},
                           Problem{Hs, U0, V, W, maxA, one_minus_gauss, forbidden_states, forbidden_coeffs, Vs}, out);
}

int qoc_create_fleet(const qoc_config* cfg, const qoc_ensemble* ens, const qoc_fleet* fleet, const qoc_transfer* tr, const qoc_control_map* map,
                     const double* Hs, const double* U0, const double* V, const double* W, const double* maxA, const double* one_minus_gauss,
                     const int32_t* forbidden_states, const double* forbidden_coeffs, const double* Vs, qoc_handle* out) {
    if (!fleet) return check_fleet("qoc_create_fleet", cfg, fleet, maxA, 1, 0);  // (refused there: a null argument, or the fleet named as missing)
    return create_composed("qoc_create_fleet", cfg, Glue{ens, fleet, tr, map},
                           Problem{Hs, U0, V, W, maxA, one_minus_gauss, forbidden_states, forbidden_coeffs, Vs}, out);
}

// an open engine through the funnel (`who`: qoc_create_open_fleet or qoc_create_open_costs): the open engine's own refusals and the running costs
// (null, or n_obs = 0: none) are checked here, the decay rides in Problem; the table of rate scales is checked with the members it has a row for
static int create_open_composed(const char* who, const qoc_config* cfg, const qoc_decay* decay, const qoc_running_costs* costs, const Glue& g,
                                const double* Hs, const double* U0, const double* V, const double* W, const double* maxA,
                                const double* one_minus_gauss, qoc_handle* out) {
    if (!cfg || !decay || !Hs || !V || !W || !maxA || !out) return fail(QOC_ERR_INVALID, "%s: null argument", who);
    const int c = decay->n_collapse;
    TRY(check_open(who, cfg, c, decay->C));
    if (costs) {
        const int nc = costs->n_obs;
        if (nc < 0 || nc > QOC_LB_MAX_COSTS) return fail(QOC_ERR_INVALID, "%s: n_obs = %d (0 .. %d running costs)", who, nc, QOC_LB_MAX_COSTS);
        if (nc > 0 && (!costs->O || !costs->coeffs || !costs->powers))
            return fail(QOC_ERR_INVALID, "%s: n_obs = %d with its observables, coefficients and powers (a null array)", who, nc);
        for (int l = 0; l < nc; ++l) {
            if (costs->powers[l] != 1 && costs->powers[l] != 2) return fail(QOC_ERR_INVALID, "%s: powers[%d] = %d (1 or 2)", who, l, costs->powers[l]);
            if (!std::isfinite(costs->coeffs[l])) return fail(QOC_ERR_INVALID, "%s: coeffs[%d] is not finite", who, l);
            const size_t per = 2 * (size_t)cfg->n * cfg->n;
            for (size_t i = 0; i < per; ++i)
                if (!std::isfinite(costs->O[per * l + i])) return fail(QOC_ERR_INVALID, "%s: observable %d is not finite", who, l);
        }
        if (nc == 0) costs = nullptr;
    }
    // (F and E bound the table of rate scales: the funnel checks them, and the table once they hold)
    DecayHost dh{c, decay->C, c > 0 ? decay->rate_scales : nullptr, g.fleet ? g.fleet->devices : 1, g.ens ? g.ens->members : 1, who};
    dh.costs = costs;
    return create_composed(who, cfg, g, Problem{Hs, U0, V, W, maxA, one_minus_gauss, nullptr, nullptr, nullptr, nullptr, &dh}, out);
}

int qoc_create_open_fleet(const qoc_config* cfg, const qoc_decay* decay, const qoc_ensemble* ens, const qoc_fleet* fleet, const qoc_transfer* tr,
                          const qoc_control_map* map, const double* Hs, const double* U0, const double* V, const double* W, const double* maxA,
                          const double* one_minus_gauss, qoc_handle* out) {
    return create_open_composed("qoc_create_open_fleet", cfg, decay, nullptr, Glue{ens, fleet, tr, map}, Hs, U0, V, W, maxA, one_minus_gauss, out);
}

// the same with running costs on expectation values (csrc/qoc_lindblad.h): the COSTS instances of the backward sweep and of the reduction
int qoc_create_open_costs(const qoc_config* cfg, const qoc_decay* decay, const qoc_running_costs* costs, const qoc_ensemble* ens, const qoc_fleet* fleet,
                          const qoc_transfer* tr, const qoc_control_map* map, const double* Hs, const double* U0, const double* V, const double* W,
                          const double* maxA, const double* one_minus_gauss, qoc_handle* out) {
    return create_open_composed("qoc_create_open_costs", cfg, decay, costs, Glue{ens, fleet, tr, map}, Hs, U0, V, W, maxA, one_minus_gauss, out);
}

// sparse operators through the funnel: the sparse engine's own refusals, the operators and the row layout are settled here.  The trajectories run
// kt + q operators; k_sp_grad forms gradients for the first kt
int qoc_create_sparse_fleet(const qoc_config* cfg, const qoc_sparse* ops, const qoc_sparse_plan* plan, const qoc_ensemble* ens, const qoc_fleet* fleet,
                            const qoc_transfer* tr, const qoc_control_map* map, const double* V, const double* W, const double* maxA,
                            const double* one_minus_gauss, const int32_t* forbidden_states, const double* forbidden_coeffs, qoc_handle* out) {
    const char* who = "qoc_create_sparse_fleet";
    if (!cfg || !ops || !V || !W || !maxA || !out) return fail(QOC_ERR_INVALID, "%s: null argument", who);
    const int layout = plan ? plan->row_layout : 0;
    if (layout < 0 || layout > 2) return fail(QOC_ERR_INVALID, "%s: row_layout = %d (0 auto, 1 per operator, 2 merged)", who, layout);
    if (ens && ens->P) return fail(QOC_ERR_INVALID, "%s: ens->P must be NULL (the perturbation operators are the last n_perturb of ops)", who);
    const int E = ens ? ens->members : 1, q = ens ? ens->n_perturb : 0;
    if (E < 1 || q < 0) return fail(QOC_ERR_INVALID, "%s: members = %d (>= 1), n_perturb = %d (>= 0)", who, E, q);
    // (the number of operators comes from the map: checked here, ahead of the operators, and -- the check is pure -- once more in the funnel)
    if (map) TRY(check_map(who, cfg, map, maxA));
    const int kt = map ? map->n_terms : cfg->k;
    if (kt < 1 || (long long)kt + q + 1 > (1 << 20)) return fail(QOC_ERR_INVALID, "%s: %d + %d + 1 operators", who, kt, q);
    const int K = kt + q + 1;
    const bool can_merge = K <= QOC_MERGE_MAX_OPS && (long long)cfg->n < (1LL << QOC_MERGE_COL_BITS);
    if (layout == 2 && K > QOC_MERGE_MAX_OPS)
        return fail(QOC_ERR_INVALID, "%s: row_layout = 2 (merged) packs the operator index into 8 bits: %d operators, at most %d", who, K, QOC_MERGE_MAX_OPS);
    if (layout == 2 && !can_merge)
        return fail(QOC_ERR_INVALID, "%s: row_layout = 2 (merged) packs the column into %d bits: n = %d, below %d", who, QOC_MERGE_COL_BITS, cfg->n, 1 << QOC_MERGE_COL_BITS);
    SparseHost sh;
    TRY(check_sparse(who, cfg, ops, K, sh));
    sh.fleet_entry = true;
    sh.kgrad = kt;
    sh.merged = layout == 2 || (layout == 0 && can_merge && QOC_SP_MERGED_AUTO(cfg->n, K));
    // (the LDS home asked for: the merged sweeps keep their coefficient table beside the vectors)
    if (sh.merged && ops->vector_home == 1 && cfg->n > qoc_sp_lds_max_n(qoc_sp_tab_bytes(K)))
        return fail(QOC_ERR_INVALID, "%s: vector_home = 1 (LDS) needs 2 n 16 bytes + %zu bytes of coefficients <= 159 KiB (n = %d, at most %d with %d merged operators)",
                    who, qoc_sp_tab_bytes(K), cfg->n, qoc_sp_lds_max_n(qoc_sp_tab_bytes(K)), K);
    if (sh.merged) {
        std::string why;
        if (!qoc_ell_merge(cfg->n, sh.ops, sh.rows, why)) return fail(QOC_ERR_INVALID, "%s: the merged rows: %s", who, why.c_str());
    }
    return create_composed(who, cfg, Glue{ens, fleet, tr, map},
                           Problem{nullptr, nullptr, V, W, maxA, one_minus_gauss, forbidden_states, forbidden_coeffs, nullptr, &sh}, out);
}

int qoc_destroy(qoc_handle e) {
    if (!e) return QOC_OK;
    hipSetDevice(e->cfg.device);
    if (e->stream) hipStreamSynchronize(e->stream);
    qoc_comm_detach(e->gm.ts_comm);                    // (a time-sharded engine: its communicator may be destroyed from now on)
    qoc_gemm_teardown(e->gm);
    for (void* p : e->allocs) hipFree(p);
    for (hipEvent_t x : e->ev) hipEventDestroy(x);
    if (e->t0) hipEventDestroy(e->t0);
    if (e->t1) hipEventDestroy(e->t1);
    if (e->stream) hipStreamDestroy(e->stream);
    delete e;
    return QOC_OK;
}

#define CHECK_H(h) if (!(h)) return fail(QOC_ERR_INVALID, "null handle"); HIP_TRY(hipSetDevice((h)->cfg.device))

int qoc_set_base(qoc_handle e, const double* base) {
    CHECK_H(e);
    if (!base) return fail(QOC_ERR_INVALID, "qoc_set_base: null base");
    const QocDev& d = sets(e);
    const size_t cnt = (size_t)d.B * d.k * d.steps;
    if (e->ens_E) HIP_TRY(hipMemsetAsync(e->d.done, 0, e->d.B * sizeof(int), e->stream));     // (the members' flags: k_ens_expand mirrors them)
    // everything on the engine stream (it is non-blocking: the legacy null stream orders nothing against it), then one sync so
    // that the caller may reuse `base` and the next qoc_iterate sees the cleared optimiser state
    HIP_TRY(hipMemcpyAsync(d.base, base, cnt * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemsetAsync(d.adam_m, 0, cnt * sizeof(double), e->stream));
    HIP_TRY(hipMemsetAsync(d.adam_v, 0, cnt * sizeof(double), e->stream));
    HIP_TRY(hipMemsetAsync(d.adam_t, 0, d.B * sizeof(int), e->stream));
    HIP_TRY(hipMemsetAsync(d.iters, 0, d.B * sizeof(int), e->stream));
    HIP_TRY(hipMemsetAsync(d.done, 0, d.B * sizeof(int), e->stream));
    if (e->lq.gram && e->lq.M) TRY(lbfgs_reset(e));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->evaluated = false;
    e->controls_ready = false;
    return QOC_OK;
}

int qoc_get_base(qoc_handle e, double* base) {
    CHECK_H(e);
    HIP_TRY(hipStreamSynchronize(e->stream));
    const QocDev& d = sets(e);
    HIP_TRY(hipMemcpy(base, d.base, (size_t)d.B * d.k * d.steps * sizeof(double), hipMemcpyDeviceToHost));
    return QOC_OK;
}

int qoc_get_scalars(qoc_handle e, double* loss, double* reg_loss, double* grad_squared, double* unitary_scale,
                    int32_t* iterations, int32_t* done) {
    CHECK_H(e);
    const QocDev& d = sets(e);
    if (unitary_scale) TRY(refresh_final(e));
    HIP_TRY(hipStreamSynchronize(e->stream));
    TRY(small_check(e));
    const size_t sz = (size_t)d.B * sizeof(double);
    if (loss) HIP_TRY(hipMemcpy(loss, d.loss, sz, hipMemcpyDeviceToHost));
    if (reg_loss) HIP_TRY(hipMemcpy(reg_loss, d.reg_loss, sz, hipMemcpyDeviceToHost));
    if (grad_squared) HIP_TRY(hipMemcpy(grad_squared, d.g2, sz, hipMemcpyDeviceToHost));
    if (unitary_scale && e->ens_E) {
        // a group's unitary_scale: the weighted sum of its members' (which the lazy paths form only on read-back, refresh_final above), in
        // member order as k_ens_reduce sums the losses
        const int E = e->ens_E;
        std::vector<double> us((size_t)e->d.B);
        HIP_TRY(hipMemcpy(us.data(), e->d.uscale, us.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int g = 0; g < d.B; ++g) {
            double acc = e->ens_wt[0] * us[(size_t)g * E];
            for (int m = 1; m < E; ++m) acc = acc + e->ens_wt[m] * us[(size_t)g * E + m];
            unitary_scale[g] = acc;
        }
    } else if (unitary_scale) HIP_TRY(hipMemcpy(unitary_scale, d.uscale, sz, hipMemcpyDeviceToHost));
    if (iterations) HIP_TRY(hipMemcpy(iterations, d.iters, d.B * sizeof(int), hipMemcpyDeviceToHost));
    if (done) HIP_TRY(hipMemcpy(done, d.done, d.B * sizeof(int), hipMemcpyDeviceToHost));
    return QOC_OK;
}

int qoc_eval(qoc_handle e, double* loss, double* reg_loss, double* grad_squared, double* unitary_scale, double* grad) {
    CHECK_H(e);
    QocAdamDev ap;
    memset(&ap, 0, sizeof ap);
    ap.mode = 0;
    TRY(enqueue_iteration(e, ap));
    TRY(qoc_get_scalars(e, loss, reg_loss, grad_squared, unitary_scale, nullptr, nullptr));
    const QocDev& d = sets(e);
    if (grad) HIP_TRY(hipMemcpy(grad, d.grad, (size_t)d.B * d.k * d.steps * sizeof(double), hipMemcpyDeviceToHost));
    return QOC_OK;
}

int qoc_adam_step(qoc_handle e, const double* lr) {
    CHECK_H(e);
    if (!lr) return fail(QOC_ERR_INVALID, "qoc_adam_step: null lr");
    if (!e->evaluated) return fail(QOC_ERR_STATE, "qoc_adam_step: no evaluation since the last qoc_set_base");
    // per-seed learning rates live in the engine's arena (no allocation per step); the copy is ordered on the engine stream
    HIP_TRY(hipMemcpyAsync(e->step_lr, lr, sets(e).B * sizeof(double), hipMemcpyHostToDevice, e->stream));
    QocAdamDev ap;
    memset(&ap, 0, sizeof ap);
    ap.mode = 2;
    ap.lr = e->step_lr;
    // the reference re-evaluates the gradient at the same parameters inside session.run([optimizer]) (run_session.py:69)
    TRY(enqueue_iteration(e, ap));
    HIP_TRY(hipStreamSynchronize(e->stream));                       // `lr` (pageable host memory) may be reused by the caller
    return QOC_OK;
}

int qoc_iterate(qoc_handle e, const qoc_adam_params* p, int32_t iters) {
    CHECK_H(e);
    if (!p) return fail(QOC_ERR_INVALID, "qoc_iterate: null params");
    const QocAdamDev ap = loop_params(p);
    if (e->path == QOC_PATH_SMALL) return iters > 0 ? enqueue_small(e, ap, iters) : QOC_OK;   // the loop runs inside the launch
    for (int i = 0; i < iters; ++i) TRY(enqueue_iteration(e, ap));
    return QOC_OK;
}

int qoc_sync(qoc_handle e) {
    CHECK_H(e);
    HIP_TRY(hipStreamSynchronize(e->stream));
    TRY(small_check(e));
    return QOC_OK;
}

int qoc_run_adam(qoc_handle e, const qoc_adam_params* p, int32_t* iterations_out) {
    CHECK_H(e);
    if (!p) return fail(QOC_ERR_INVALID, "qoc_run_adam: null params");
    const QocAdamDev ap = loop_params(p);
    // at most max_iterations updates + the evaluation that trips the stop rule
    return run_until_done(e, "qoc_run_adam", "seeds", (long long)p->max_iterations + 1, p->poll_every, iterations_out, [&](int burst) -> int {
        if (e->path == QOC_PATH_SMALL) return enqueue_small(e, ap, burst);       // (one launch per burst)
        for (int i = 0; i < burst; ++i) TRY(enqueue_iteration(e, ap));
        return QOC_OK;
    });
}

int qoc_iterate_lbfgs(qoc_handle e, const qoc_lbfgs_params* p, int32_t iters) {
    CHECK_H(e);
    QocLbfgsDev L;
    TRY(lbfgs_prepare(e, p, "qoc_iterate_lbfgs", &L));
    for (int i = 0; i < iters; ++i) TRY(enqueue_lbfgs_iteration(e, L));
    return QOC_OK;
}

int qoc_run_lbfgs(qoc_handle e, const qoc_lbfgs_params* p, int32_t* iterations_out) {
    CHECK_H(e);
    QocLbfgsDev L;
    TRY(lbfgs_prepare(e, p, "qoc_run_lbfgs", &L));
    // at most max_iterations evaluations that move the variable, one whose trial is refused at the limit, one of the accepted point restored
    return run_until_done(e, "qoc_run_lbfgs", "control sets", (long long)p->max_iterations + 2, p->poll_every, iterations_out, [&](int burst) -> int {
        for (int i = 0; i < burst; ++i) TRY(enqueue_lbfgs_iteration(e, L));
        return QOC_OK;
    });
}

int qoc_get_uks(qoc_handle e, double* uks) {
    CHECK_H(e);
    if (!uks) return fail(QOC_ERR_INVALID, "qoc_get_uks: null output");
    const QocDev& d = sets(e);
    // uks = maxA[k] * sin(base) of the CURRENT variable (run_session.py:112-117), evaluated on the device
    const int total = d.B * d.k * d.steps;
    // (into u2 / w2: u / w keep the controls of the last evaluation for qoc_get_uks_evaluated and the regularisers' read-backs)
    if (!e->controls_ready) {
        QocDev dd = d;
        dd.u = d.u2; dd.w = d.w2;
        launch_controls(dd, e->stream);
        HIP_TRY(hipGetLastError());
        e->controls_ready = true;
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(uks, d.u2, (size_t)total * sizeof(double), hipMemcpyDeviceToHost));
    return QOC_OK;
}

int qoc_get_uks_evaluated(qoc_handle e, double* uks) {
    CHECK_H(e);
    if (!uks) return fail(QOC_ERR_INVALID, "qoc_get_uks_evaluated: null output");
    if (!e->evaluated) return fail(QOC_ERR_STATE, "qoc_get_uks_evaluated: nothing evaluated yet");
    // d.u still holds the controls the last evaluation ran on (an Adam step only moves `base`)
    HIP_TRY(hipStreamSynchronize(e->stream));
    const QocDev& d = sets(e);
    HIP_TRY(hipMemcpy(uks, d.u, (size_t)d.B * d.k * d.steps * sizeof(double), hipMemcpyDeviceToHost));
    return QOC_OK;
}

int qoc_get_pulse(qoc_handle e, double* u) {
    CHECK_H(e);
    if (!e->shaped) return fail(QOC_ERR_STATE, "qoc_get_pulse: not a shaped engine (qoc_create_shaped)");
    if (!u) return fail(QOC_ERR_INVALID, "qoc_get_pulse: null output");
    if (!e->evaluated) return fail(QOC_ERR_STATE, "qoc_get_pulse: nothing evaluated yet");
    // (k_shape_expand stores the nominal pulse of every evaluation beside the trajectories' scaled copies)
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(u, e->sh.uf, (size_t)e->g.B * e->g.k * e->d.steps * sizeof(double), hipMemcpyDeviceToHost));
    return QOC_OK;
}

// a per-trajectory array read back per control set: the first `bytes` of every trajectory's `stride` bytes, of every trajectory on a plain engine
// (bytes = stride there) and of member 0 of each control set on an ensemble engine
static int copy_out_sets(const qoc_engine* e, void* dst, const void* src, size_t bytes, size_t stride) {
    if (e->ens_E) HIP_TRY(hipMemcpy2D(dst, bytes, src, stride * e->ens_E, bytes, (size_t)e->g.B, hipMemcpyDeviceToHost));
    else HIP_TRY(hipMemcpy(dst, src, (size_t)e->d.B * bytes, hipMemcpyDeviceToHost));
    return QOC_OK;
}

int qoc_get_coefficients(qoc_handle e, double* c) {
    CHECK_H(e);
    if (!e->mapped) return fail(QOC_ERR_STATE, "qoc_get_coefficients: not a mapped engine (qoc_create_mapped)");
    if (!c) return fail(QOC_ERR_INVALID, "qoc_get_coefficients: null output");
    if (!e->evaluated) return fail(QOC_ERR_STATE, "qoc_get_coefficients: nothing evaluated yet");
    // (the first r rows of member 0's trajectory: what k_map_expand wrote for the last evaluation)
    HIP_TRY(hipStreamSynchronize(e->stream));
    return copy_out_sets(e, c, e->d.u, (size_t)e->cm.r * e->d.steps * sizeof(double), (size_t)e->d.k * e->d.steps * sizeof(double));
}

int qoc_get_final_unitary(qoc_handle e, double* Uf) {
    CHECK_H(e);
    if (e->lb.on) return fail(QOC_ERR_STATE, "qoc_get_final_unitary: an open engine has no final unitary (qoc_get_final_density)");
    if (e->d.state_transfer) return fail(QOC_ERR_STATE, "qoc_get_final_unitary: state-transfer mode has no final unitary");
    if (!e->evaluated) return fail(QOC_ERR_STATE, "qoc_get_final_unitary: nothing evaluated yet");
    TRY(refresh_final(e));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const size_t row = (size_t)e->d.n * e->d.n * sizeof(cplx);
    return copy_out_sets(e, Uf, e->d.Xfinal, row, row);
}

int qoc_get_inter_vecs(qoc_handle e, double* inter) {
    CHECK_H(e);
    if (e->lb.on) return fail(QOC_ERR_STATE, "qoc_get_inter_vecs: an open engine propagates no state vectors (qoc_get_populations)");
    if (!e->evaluated) return fail(QOC_ERR_STATE, "qoc_get_inter_vecs: nothing evaluated yet");
    // one rank of a time-sharded run: its own slices, summed over the ranks (a collective)
    if (e->path == QOC_PATH_GEMM) TRY(qoc_gemm_ts_gather_inter(e->gm, e->d, e->stream));
    if (e->path == QOC_PATH_SMALL) TRY(refresh_small(e, true));
    else if (e->inter_stale) {                                       // latency mode: the sweeps keep Psi_t in their own layout
        qoc_mfma_unpack_inter(e->mp, e->mf, e->d, e->stream);
        HIP_TRY(hipGetLastError());
        e->inter_stale = false;
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    const size_t row = (size_t)(e->d.steps + 1) * e->d.n * e->d.m * sizeof(cplx);
    return copy_out_sets(e, inter, e->d.inter, row, row);
}

// rho_ij(T) of trajectory b, [m][m][n][n] complex: the pairs i > j mirrored from rho_ji
static int read_density(qoc_engine* e, size_t b, double* rho) {
    const QocDev& d = e->d;
    const int n = d.n, m = d.m, R = e->lb.R;
    const size_t nn = (size_t)n * n;
    std::vector<cplx> blk(nn);
    for (int i = 0, r = 0; i < m; ++i)
        for (int j = i; j < m; ++j, ++r) {
            HIP_TRY(hipMemcpy(blk.data(), e->lb.hist + ((b * R + r) * d.steps + (d.steps - 1)) * nn, nn * sizeof(cplx), hipMemcpyDeviceToHost));
            double* up = rho + 2 * (((size_t)i * m + j) * nn);
            double* lo = rho + 2 * (((size_t)j * m + i) * nn);
            for (int a = 0; a < n; ++a)
                for (int c = 0; c < n; ++c) {
                    const cplx v = blk[(size_t)a * n + c];
                    up[2 * (a * n + c)] = v.x; up[2 * (a * n + c) + 1] = v.y;
                    if (i != j) { lo[2 * (c * n + a)] = v.x; lo[2 * (c * n + a) + 1] = -v.y; }   // rho_ji = rho_ij^dagger
                }
        }
    return QOC_OK;
}

int qoc_get_final_density(qoc_handle e, double* rho) {
    CHECK_H(e);
    if (!e->lb.on) return fail(QOC_ERR_STATE, "qoc_get_final_density: not an open engine (qoc_create_open)");
    if (!rho) return fail(QOC_ERR_INVALID, "qoc_get_final_density: null output");
    if (!e->evaluated) return fail(QOC_ERR_STATE, "qoc_get_final_density: nothing evaluated yet");
    HIP_TRY(hipStreamSynchronize(e->stream));
    const size_t per = 2 * (size_t)e->d.m * e->d.m * e->d.n * e->d.n, E = e->ens_E ? (size_t)e->ens_E : 1;      // (an ensemble: member 0 of each control set)
    for (size_t g = 0; g < (size_t)sets(e).B; ++g) TRY(read_density(e, g * E, rho + g * per));
    return QOC_OK;
}

int qoc_get_member_final_density(qoc_handle e, double* rho) {
    CHECK_H(e);
    if (!e->lb.on || !e->ens_E) return fail(QOC_ERR_STATE, "qoc_get_member_final_density: not an open ensemble engine (qoc_create_open_fleet)");
    if (!rho) return fail(QOC_ERR_INVALID, "qoc_get_member_final_density: null output");
    if (!e->evaluated) return fail(QOC_ERR_STATE, "qoc_get_member_final_density: nothing evaluated yet");
    HIP_TRY(hipStreamSynchronize(e->stream));
    const size_t per = 2 * (size_t)e->d.m * e->d.m * e->d.n * e->d.n;
    for (size_t b = 0; b < (size_t)e->d.B; ++b) TRY(read_density(e, b, rho + b * per));
    return QOC_OK;
}

int qoc_get_populations(qoc_handle e, double* pop) {
    CHECK_H(e);
    if (!e->lb.on) return fail(QOC_ERR_STATE, "qoc_get_populations: not an open engine (qoc_create_open)");
    if (!pop) return fail(QOC_ERR_INVALID, "qoc_get_populations: null output");
    if (!e->evaluated) return fail(QOC_ERR_STATE, "qoc_get_populations: nothing evaluated yet");
    const QocDev& d = e->d;
    const size_t row = (size_t)(d.steps + 1) * d.n * d.m, total = (size_t)d.B * row;
    hipLaunchKernelGGL(k_lb_populations, dim3(grid_for(total, QOC_BLOCK, 2048)), dim3(QOC_BLOCK), 0, e->stream, d, e->lb);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    return copy_out_sets(e, pop, e->lb.pop, row * sizeof(double), row * sizeof(double));
}

int qoc_get_expectations(qoc_handle e, double* x) {
    CHECK_H(e);
    if (!e->lb.on || e->lb.nc < 1) return fail(QOC_ERR_STATE, "qoc_get_expectations: not an open engine with running costs (qoc_create_open_costs)");
    if (!x) return fail(QOC_ERR_INVALID, "qoc_get_expectations: null output");
    if (!e->evaluated) return fail(QOC_ERR_STATE, "qoc_get_expectations: nothing evaluated yet");
    const QocDev& d = e->d;
    const size_t row = (size_t)(d.steps + 1) * e->lb.nc * d.m;
    hipLaunchKernelGGL(k_lb_expectations, dim3((unsigned)((size_t)d.B * (d.steps + 1))), dim3(QOC_BLOCK), 0, e->stream, d, e->lb);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    return copy_out_sets(e, x, e->lb.expct, row * sizeof(double), row * sizeof(double));
}

int qoc_get_member_scalars(qoc_handle e, double* loss, double* reg_state) {
    CHECK_H(e);
    if (!e->ens_E) return fail(QOC_ERR_STATE, "qoc_get_member_scalars: not an ensemble engine (qoc_create_ensemble)");
    if (!e->evaluated) return fail(QOC_ERR_STATE, "qoc_get_member_scalars: nothing evaluated yet");
    HIP_TRY(hipStreamSynchronize(e->stream));
    const size_t sz = (size_t)e->d.B * sizeof(double);
    if (loss) HIP_TRY(hipMemcpy(loss, e->d.loss, sz, hipMemcpyDeviceToHost));
    if (reg_state) HIP_TRY(hipMemcpy(reg_state, e->d.reg_state, sz, hipMemcpyDeviceToHost));
    return QOC_OK;
}

// the weights every control set starts from: the members' own
static int risk_fill_weights(qoc_engine* e) {
    const size_t E = (size_t)e->ens_E;
    std::vector<double> w((size_t)e->g.B * E);
    for (size_t i = 0; i < w.size(); ++i) w[i] = e->ens_wt[i % E];
    HIP_TRY(hipMemcpy(e->risk_pi, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
    return QOC_OK;
}

int qoc_set_risk(qoc_handle e, double beta) {
    CHECK_H(e);
    if (!e->ens_E) return fail(QOC_ERR_STATE, "qoc_set_risk: not an ensemble engine (qoc_create_ensemble, qoc_create_shaped)");
    if (std::isnan(beta)) return fail(QOC_ERR_INVALID, "qoc_set_risk: beta is NaN");
    if (std::isinf(beta)) return fail(QOC_ERR_INVALID, "qoc_set_risk: beta is infinite (a hard maximum is the limit of large finite beta)");
    if (beta < 0.0) return fail(QOC_ERR_INVALID, "qoc_set_risk: beta = %g is negative (>= 0; 0 is the weighted mean)", beta);
    HIP_TRY(hipStreamSynchronize(e->stream));            // (the evaluations enqueued so far keep the beta they were enqueued with)
    if (beta > 0.0 && !e->risk_pi) TRY(dev_alloc(e, &e->risk_pi, (size_t)e->g.B * e->ens_E));
    // leaving the mean: a control set that is not evaluated again (finished in a loop) holds the members' own weights
    if (beta > 0.0 && e->risk_beta == 0.0) TRY(risk_fill_weights(e));
    e->risk_beta = beta;
    return QOC_OK;
}

int qoc_set_traces(qoc_handle e, const double* traces) {
    CHECK_H(e);
    if (!e->ens_E)
        return fail(QOC_ERR_STATE, "qoc_set_traces: the engine has no member table (qoc_create, qoc_create_open and qoc_create_sparse make none; "
                                   "qoc_create_ensemble and the entry points after it do)");
    if (e->en.q < 1) return fail(QOC_ERR_STATE, "qoc_set_traces: the members have no perturbation row to add a trace to (q = 0)");
    const size_t F = e->fleet_F ? (size_t)e->fleet_F : 1;
    const size_t cnt = F * (size_t)e->ens_E * (size_t)e->en.q * (size_t)e->d.steps;
    if (traces)
        for (size_t i = 0; i < cnt; ++i)
            if (!std::isfinite(traces[i])) return fail(QOC_ERR_INVALID, "qoc_set_traces: entry %zu of the table is not finite", i);
    HIP_TRY(hipStreamSynchronize(e->stream));            // (the evaluations enqueued so far keep the table they were enqueued with)
    if (!traces) { e->en.tr = nullptr; return QOC_OK; }  // (the device copy stays for a later table)
    if (!e->traces) TRY(dev_alloc(e, &e->traces, cnt));
    HIP_TRY(hipMemcpy(e->traces, traces, cnt * sizeof(double), hipMemcpyHostToDevice));
    e->en.tr = e->traces;
    return QOC_OK;
}

int qoc_get_member_weights(qoc_handle e, double* pi) {
    CHECK_H(e);
    if (!e->ens_E) return fail(QOC_ERR_STATE, "qoc_get_member_weights: not an ensemble engine (qoc_create_ensemble, qoc_create_shaped)");
    if (!pi) return fail(QOC_ERR_INVALID, "qoc_get_member_weights: null output");
    const size_t E = (size_t)e->ens_E, cnt = (size_t)e->g.B * E;
    if (!risk_on(e)) {
        for (size_t i = 0; i < cnt; ++i) pi[i] = e->ens_wt[i % E];
        return QOC_OK;
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(pi, e->risk_pi, cnt * sizeof(double), hipMemcpyDeviceToHost));
    return QOC_OK;
}

int qoc_get_trajectory_gradient(qoc_handle e, double* dLdu) {
    CHECK_H(e);
    if (!e->ens_E) return fail(QOC_ERR_STATE, "qoc_get_trajectory_gradient: not an ensemble engine (qoc_create_ensemble)");
    if (!dLdu) return fail(QOC_ERR_INVALID, "qoc_get_trajectory_gradient: null output");
    if (!e->evaluated) return fail(QOC_ERR_STATE, "qoc_get_trajectory_gradient: nothing evaluated yet");
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(dLdu, e->d.dLdu, (size_t)e->d.B * e->d.k * e->d.steps * sizeof(double), hipMemcpyDeviceToHost));
    return QOC_OK;
}

int qoc_get_member_final_unitary(qoc_handle e, double* Uf) {
    CHECK_H(e);
    if (!e->ens_E) return fail(QOC_ERR_STATE, "qoc_get_member_final_unitary: not an ensemble engine (qoc_create_ensemble)");
    if (e->lb.on) return fail(QOC_ERR_STATE, "qoc_get_member_final_unitary: an open engine has no final unitary (qoc_get_member_final_density)");
    if (!Uf) return fail(QOC_ERR_INVALID, "qoc_get_member_final_unitary: null output");
    if (e->d.state_transfer) return fail(QOC_ERR_STATE, "qoc_get_member_final_unitary: state-transfer mode has no final unitary");
    if (!e->evaluated) return fail(QOC_ERR_STATE, "qoc_get_member_final_unitary: nothing evaluated yet");
    TRY(refresh_final(e));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(Uf, e->d.Xfinal, (size_t)e->d.B * e->d.n * e->d.n * sizeof(cplx), hipMemcpyDeviceToHost));
    return QOC_OK;
}

int qoc_profile_enable(qoc_handle e, int32_t on) {
    CHECK_H(e);
    TRY(prof_collect(e));
    e->profiling = on != 0;
    e->prof_ms = 0.0;
    e->prof_launches = 0;
    return QOC_OK;
}

int qoc_profile_read(qoc_handle e, const char** kernel_name, int64_t* launches, double* total_ms) {
    CHECK_H(e);
    TRY(prof_collect(e));
    if (kernel_name)
        *kernel_name = e->path == QOC_PATH_SPARSE ? "k_sp_forward" : e->path == QOC_PATH_LINDBLAD ? "k_lb_forward" : e->path == QOC_PATH_LINDBLAD_TILED ? "k_lbt_forward" : e->path == QOC_PATH_SMALL ? "k_small_iter (whole iterations)"
                       : e->path == QOC_PATH_GEMM ? (e->gm.route == QOC_GEMM_DIRECT ? "k_gemm_taylor_chain (backward chain + sources + gradient products)"
                           : e->gm.N <= 64 ? "k_gemm_expm_fused (+ product tree)" : "k_zgemm_wg + k_zgemm32 (batched matexp sequence)")
                       : e->path == QOC_PATH_MFMA ? e->mp.expm_name             // (the kernel of the exponentials, by its variant)
                       : e->path == QOC_PATH_ST_FUSED ? "k_st_fwd_fused" : (e->d.state_transfer ? "k_st_fwd_generic" : "k_expm_generic");
    if (launches) *launches = e->prof_launches;
    if (total_ms) *total_ms = e->prof_ms;
    return QOC_OK;
}

int qoc_time_iterations(qoc_handle e, const qoc_adam_params* p, int32_t iters, double* elapsed_ms) {
    CHECK_H(e);
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipEventRecord(e->t0, e->stream));
    TRY(qoc_iterate(e, p, iters));
    HIP_TRY(hipEventRecord(e->t1, e->stream));
    HIP_TRY(hipEventSynchronize(e->t1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->t0, e->t1));
    if (elapsed_ms) *elapsed_ms = ms;
    return QOC_OK;
}

int qoc_path_in_use(qoc_handle e) { return e ? e->path : QOC_ERR_INVALID; }
int qoc_chunks_in_use(qoc_handle e) { return e ? e->chunks : QOC_ERR_INVALID; }

// What AUTO resolved to, as one line of key=value pairs (tests/test_auto_plan.py pins the dispatch table of DESIGN.md section 4 with it):
// MFMA path:  path=mfma nt=<tiles> expm=<exponential kernel 1..8> chunks=<C> [expm=8: expm_hermitian=<0|1|2>: plain Horner chain | S S with copied accumulators | even/odd chain of symmetric products]
// mem_policy=<0|1: plain accesses | the policy instances of k_mfma_expm_inplace / k_mfma_downup (qoc_mfma_frag.h, QocMem); same bits>
// sweeps=<downup|split|row_tile_gradient|latency|latency_sources|one_wave>
//   GEMM path:  path=gemm route=<unitary|propagator|direct> chunks=<NC> slices_per_chunk=<S> chains=<persistent|launches>
//   others:     path=generic | path=st_fused
//   open engines (qoc_create_open, qoc_create_open_fleet): path=lindblad collapse=<c> pairs=<R> lds=<bytes of dynamic LDS>
//   the same with cfg.path = QOC_PATH_LINDBLAD_TILED: path=lindblad_tiled collapse=<c> pairs=<R> np=<NP> work=<bytes of the workgroups' scratch>
//   (qoc_create_open_costs with n_obs > 0 ends the line with running_costs=<L>)
//   sparse engines (qoc_create_sparse): path=sparse nnz=<stored entries> ell=<W_0,..,W_k> vector_home=<lds|global> lds=<bytes of dynamic LDS> threads=<256|1024 of a sweep>
//   grad_grid=<workgroups of k_sp_grad>; engines of qoc_create_sparse_fleet add rows=<per_operator|merged> merged_width=<Wm, 0 per operator>
// on every path gradient=<first_order|exact> (qoc_config.gradient), and tail=<finish256_regs|finish256_memory|finish1024_regs|finish1024_regs8|finish1024_memory|split<S>[_partials]|latency_fused_regs|latency_fused_memory|in_launch>
// exact engines add exact_variant=<lds|global> exact_lds=<bytes of dynamic LDS, 0 in the global variant> exact_grid=<workgroups of k_exact_grad>
int qoc_plan_describe(qoc_handle e, char* buf, int32_t len) {
    if (!e || !buf || len < 1) return fail(QOC_ERR_INVALID, "qoc_plan_describe: null handle or buffer");
    char tmp[768];
    if (e->path == QOC_PATH_MFMA) {
        int w = snprintf(tmp, sizeof tmp, "path=mfma nt=%d expm=%d chunks=%d sweeps=%s", e->mf.NT, e->mp.expm_variant, e->mf.C, e->mp.sweeps);
        // the in-place exponential kernel only: what it makes of exactly anti-Hermitian generators (Taylor order 5, 29 <= n <= 32; qoc_mfma_plan.h)
        if (e->mp.expm_variant == 8) w += snprintf(tmp + w, sizeof tmp - w, " expm_hermitian=%d", e->mp.expm_hermitian);
        // how k_mfma_expm_inplace and k_mfma_downup request their K and X streams (QocMfmaPlan::mem_policy): 0 plain accesses, 1 the policy instances
        snprintf(tmp + w, sizeof tmp - w, " mem_policy=%d", e->mp.mem_policy);
    } else if (e->path == QOC_PATH_GEMM) {
        const QocGemm& g = e->gm;
        const bool direct = g.route == QOC_GEMM_DIRECT;
        int w = snprintf(tmp, sizeof tmp, "path=gemm route=%s chunks=%d slices_per_chunk=%d chains=%s",
                         direct ? "direct" : (e->d.state_transfer ? "propagator" : "unitary"), g.NC, g.S, qoc_gemm_chain_routes(g) ? "persistent" : "launches");
        if (g.ts_G > 0) w += snprintf(tmp + w, sizeof tmp - w, " time_shards=%d time_rank=%d", g.ts_G, g.ts_rank);
        // the kernel of the direct route's Taylor chains: squared (k_gemm_taylor_chain_sq on [B | B^2]), packed / full
        // (k_gemm_taylor_chain_dpp), butterfly (k_gemm_taylor_chain)
        if (direct) snprintf(tmp + w, sizeof tmp - w, " taylor_chain=%s",
                             g.sq_chain ? "squared" : g.dpp_packed ? "packed"
                             : g.dpp_chain ? (g.dpp_cw == 10 ? "columns40" : g.dpp_cw == 12 ? "columns48" : g.dpp_cw == 14 ? "columns56" : "full")
                             : "butterfly");
    } else if (e->path == QOC_PATH_LINDBLAD) {
        snprintf(tmp, sizeof tmp, "path=lindblad collapse=%d pairs=%d lds=%zu", e->lb.c, e->lb.R, e->lb.lds_bytes);
    } else if (e->path == QOC_PATH_LINDBLAD_TILED) {
        snprintf(tmp, sizeof tmp, "path=lindblad_tiled collapse=%d pairs=%d np=%d work=%zu", e->lb.c, e->lb.R, e->lbt.NP, e->lbt.work_bytes);
    } else if (e->path == QOC_PATH_SPARSE) {
        const QocSparse& sp = e->sp;
        int w = snprintf(tmp, sizeof tmp, "path=sparse nnz=%lld ell=", sp.stored);
        for (size_t j = 0; j < e->sp_widths.size() && w < 320; ++j) w += snprintf(tmp + w, sizeof tmp - w, j ? ",%d" : "%d", e->sp_widths[j]);
        w += snprintf(tmp + w, sizeof tmp - w, " vector_home=%s lds=%zu threads=%d grad_grid=%d", sp.home == 1 ? "lds" : "global", sp.lds_bytes, sp.threads, sp.grad_grid);
        // engines of qoc_create_sparse_fleet only (the line of qoc_create_sparse stays as it was)
        if (e->sp_fleet_entry) snprintf(tmp + w, sizeof tmp - w, " rows=%s merged_width=%d", sp.merged ? "merged" : "per_operator", sp.Wm);
    } else if (e->path == QOC_PATH_SMALL) {
        snprintf(tmp, sizeof tmp, "path=small n_pad=%d rows=%d slices_per_row=%d workgroups=%d state_sources=%d lds_kb=%d", e->sm.N, e->sm.R, e->sm.L, e->sm.G,
            e->sm.src ? 1 : 0, (int)((e->sm.lds_bytes + 1023) / 1024));
    } else {
        snprintf(tmp, sizeof tmp, "path=%s", e->path == QOC_PATH_ST_FUSED ? "st_fused" : "generic");
    }
    // the kernel of the Adam tail (tail_kind) and where its elements live: registers while ks <= QFE x threads (finish_body's in_regs)
    auto add = [&tmp](const char* fmt, auto... a) { const size_t w = strlen(tmp); snprintf(tmp + w, sizeof tmp - w, fmt, a...); };
    const int ks = sets(e).k * sets(e).steps;
    const TailKind tail = tail_kind(e);
    if (tail == TAIL_IN_LAUNCH) add(" tail=%s", "in_launch");
    else if (tail == TAIL_SPLIT) add(" tail=split%d", e->fin_S);
    else if (tail == TAIL_SPLIT_PARTIALS) add(" tail=split%d_partials", e->fin_S);
    else if (tail == TAIL_LATENCY_FUSED) add(" tail=latency_fused_%s", ks <= QF_E * (int)e->mp.grad_lat.block.x ? "regs" : "memory");
    else {
        const int threads = ks >= 2048 ? 1024 : QOC_BLOCK, qfe = tail == TAIL_FINISH8 ? 8 : QF_E;
        add(" tail=finish%d_%s", threads, tail == TAIL_FINISH8 ? "regs8" : (ks <= qfe * threads ? "regs" : "memory"));
    }
    // ensemble engines only (the plain engines' line stays as it was)
    if (e->ens_E) add(" members=%d perturbations=%d", e->ens_E, e->en.q);
    if (e->fleet_F) add(" devices=%d", e->fleet_F);
    if (e->shaped) add(" samples=%d band=%d", e->sh.P, e->sh.band);
    if (e->mapped) add(" terms=%d degree=%d", e->cm.r, e->cm.D);
    add(" gradient=%s", e->xg.on ? "exact" : "first_order");
    // exact engines only: where k_exact_grad keeps its generator and vector blocks, its dynamic LDS and its grid (qoc_exact_plan)
    if (e->xg.on) add(" exact_variant=%s exact_lds=%zu exact_grid=%d", e->xg.lds ? "lds" : "global", e->xg.lds_bytes, e->xg.grid);
    // open engines with running costs only (qoc_create_open_costs)
    if (e->lb.on && e->lb.nc > 0) add(" running_costs=%d", e->lb.nc);
    // while a trace table is set only (qoc_set_traces)
    if (e->en.tr) add(" traces=1");
    snprintf(buf, (size_t)len, "%s", tmp);
    return QOC_OK;
}

}  // extern "C"

#include "qoc_comm.h"
