/*
 * qoc.h -- C ABI of the MI355X-native GRAPE engine (libqoc_hip.so).
 *
 * The reference (SchusterLab/quantum-optimal-control, Python + TensorFlow 1.x) has no FFI: its "operator API" is the
 * set of tensors that core/run_session.py and core/analysis.py fetch from the TensorflowState graph.
 * Every entry point below replaces one of those fetches / feeds; the file:line cited is the reference call site,
 * relative to /root/reference/quantum_optimal_control/.
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every host buffer; the engine copies inputs to HBM at
 *     qoc_create() and owns device memory until qoc_destroy(); outputs are written into caller buffers.
 *   - complex arrays are C-order interleaved (re, im) float64, i.e. numpy complex128.
 *   - all per-seed arrays have a leading n_seeds dimension (independent random-restart control sets that share the
 *     Hamiltonians; the reference has exactly one seed per Grape() call).
 *   - every function returns QOC_OK (0) or a negative status; qoc_last_error() gives the message (thread-local).
 *   - a handle is not thread-safe; one HIP stream per handle; one process per GPU.
 */
#ifndef QOC_H
#define QOC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QOC_OK 0
#define QOC_ERR_INVALID (-1)   /* bad argument / unsupported configuration */
#define QOC_ERR_HIP (-2)       /* HIP runtime error (message has the hipError string) */
#define QOC_ERR_NOMEM (-3)
#define QOC_ERR_STATE (-4)     /* call sequence error (e.g. adam step before any evaluation) */

#define QOC_PATH_AUTO 0
#define QOC_PATH_GENERIC 1     /* any n: workgroup-cooperative complex-fp64 products from HBM/L2 */
#define QOC_PATH_MFMA 2        /* n <= 64: register-resident MFMA chain kernels (v_mfma_f64_4x4x4 / 16x16x4; AUTO for n <= 32 batches); unitary mode, and state
                                * transfer with exactly anti-Hermitian generators (K_t = sum_{j < T} A^j / j! + the same thin sweeps; AUTO up to n = 48) */
#define QOC_PATH_ST_FUSED 3    /* state transfer, n <= 64, m <= 4: register-resident generator, LDS vectors */
#define QOC_PATH_GEMM 4        /* any n, m <= 32, both modes: fused LDS exponentials + product tree + persistent thin chains (n <= 64),
                                * batched tiled MFMA GEMM launches above; state transfer by propagators or, with chunks = 1, directly */
#define QOC_PATH_SMALL 5       /* n <= 12, m <= n, k <= 8, no bandpass, <= 4 forbidden levels: the WHOLE iteration (and qoc_iterate's / qoc_run_adam's loop)
                                * inside one launch -- a row of 16 lanes per time slice, matrices column-per-lane in registers, plain complex-fp64 FMAs
                                * (v_fmac_f64_dpp), product tree in LDS, several workgroups per control set for long pulses (csrc/qoc_small.h); AUTO for
                                * one or a few control sets of the sizes the reference is used at (qubits, qutrits, two / three transmons) */
#define QOC_PATH_LINDBLAD 6    /* engines made by qoc_create_open only: n <= 32, density operators of the pairs of states of interest resident in LDS,
                                * plain complex-fp64 FMAs (csrc/qoc_lindblad.h) */

#define QOC_PATH_SPARSE 7      /* engines made by qoc_create_sparse only: state transfer on sparse operators, any n; ELLPACK mat-vecs, the state vector of a
                                * (control set, column) resident in the LDS of one compute unit up to n = 5088, in global scratch above (csrc/qoc_sparse.h) */
#define QOC_PATH_LINDBLAD_TILED 8 /* engines made by qoc_create_open* only, and only by name (AUTO stays QOC_PATH_LINDBLAD): n <= 128, any n_collapse <= 8; the
                                * operators in per-workgroup global scratch, n x n products on v_mfma_f64_16x16x4 tiles (csrc/qoc_lindblad_tiled.h) */

typedef struct qoc_engine* qoc_handle;

/* Static problem description == what SystemParameters hands to TensorflowState
 * (core/system_parameters.py:12-86 -> core/tensorflow_state.py:13-15). */
typedef struct qoc_config {
    int32_t n;              /* state_num                       system_parameters.py:165 */
    int32_t k;              /* ops_len                         system_parameters.py:202 */
    int32_t steps;          /*                                 system_parameters.py:164 */
    int32_t m;              /* len(states_concerned_list)      system_parameters.py:171 */
    int32_t taylor_terms;   /* exp_terms                       system_parameters.py:226-230 */
    int32_t scaling;        /* scaling (squarings)             system_parameters.py:226-230 */
    int32_t state_transfer; /* 0: unitary (matexp_op chain), 1: state transfer (matvecexp_op)  tensorflow_state.py:374-383 */
    int32_t n_seeds;        /* >= 1 */
    double dt;              /* total_time / steps */
    double total_time;
    /* get_reg_loss terms (core/regularization_functions.py:7-97): presence flag + coefficient (un-normalised,
     * the engine divides by steps as the reference does). */
    int32_t has_amplitude, has_envelope, has_dwdt, has_d2wdt2, has_speed_up, has_bandpass;
    double c_amplitude, c_envelope, c_dwdt, c_d2wdt2, c_speed_up, c_bandpass;
    int32_t band_lo, band_hi;   /* band_id = (band*total_time).astype(int)   regularization_functions.py:61 */
    int32_t n_forbidden;        /* len(forbidden_coeff_list)                 regularization_functions.py:71-85 */
    int32_t forbid_dressed;     /* rotate inter_vecs by sort_ev(v_c)^dagger  regularization_functions.py:73-80 */
    int32_t device;             /* HIP device ordinal */
    int32_t path;               /* QOC_PATH_* */
    int32_t chunks;             /* MFMA path: time chunks per seed (0 = auto).  GEMM path, state transfer: 1 = direct route (Taylor
                                 * mat-vec chains, any H), > 1 = propagator route (needs anti-Hermitian generators), 0 = auto.
                                 * Workgroup-resident path (QOC_PATH_SMALL): workgroups per control set (0 = auto) */
    int32_t variant;            /* MFMA path, kernel family: 0 = auto, 1 = v_mfma_f64_16x16x4 everywhere (exponentials by one wave per
                                 * 16-column block of a chunk, one-wave sweeps), 2 = v_mfma_f64_4x4x4 exponentials by one wave per
                                 * 16-column block, 3 = v_mfma_f64_4x4x4 exponentials by one wave per chunk (n <= 32; n > 32: same
                                 * as 2), 4 = as 3 with the left-operand image written under the product's own MFMAs (the round-2
                                 * default), 5 = latency mode (n <= 64; n <= 16 is padded to 32; auto
                                 * for one or a few control sets, decided by seeds x time slices: exponentials
                                 * per time slice, forward and z-free adjoint sweep side by side, slice-parallel gradient),
                                 * 6 = v_mfma_f64_4x4x4 exponentials by two waves per chunk, two waves
                                 * per SIMD (n <= 32; slower than 4, kept for A/B runs), 7 = n > 32: v_mfma_f64_4x4x4
                                 * exponentials by four waves per chunk, a block of rows each (auto for n > 32), 8 = as 4 with
                                 * row-strip-major products whose result rewrites the left-operand image in place (n <= 32, Taylor
                                 * order >= 3; auto for n <= 32 batches since round 3); 2..8 (and auto) run the n <= 32 sweeps on
                                 * v_mfma_f64_4x4x4 as well.
                                 * GEMM path requested explicitly (path = QOC_PATH_GEMM), direct state-transfer route at n in 33..64 with one
                                 * state vector and Hermitian H: 2 = the squared-generator Taylor chain (csrc/qoc_gemm_chain_sq.h; opt-in,
                                 * measured slower than the default chain), other values = the default chain.
                                 * Workgroup-resident path (QOC_PATH_SMALL): rows of 16 lanes per workgroup, 8 / 16 / 32 (0 = auto; A/B runs) */
    int32_t plan_seeds;         /* 0, or the batch size AUTO plans for instead of n_seeds: path, kernel family, chunk count and split
                                 * factors are derived from it, so that a restart evolves bit-identically whether it runs in one engine
                                 * of `plan_seeds` control sets or in a shard of it (GrapeSharded passes restarts / GPUs of the node) */
    int32_t time_shards;        /* 0: off.  G >= 1: ONE large trajectory sharded along the TIME axis over G ranks (the
                                 * alternative for config 5): rank r computes the propagators, sweeps and gradients of its run of time
                                 * chunks; two collectives per iteration (all-gather of G rank products, all-reduce of the gradient
                                 * array) on the engine's stream.  GEMM path, unitary mode, one control set, no state regulariser,
                                 * n > 96, m <= 8 (csrc/qoc_gemm_ts.h); the reference has no counterpart (single device,
                                 * main_grape/grape.py:106-109) */
    int32_t time_rank;          /* this engine's rank 0 .. time_shards - 1 (give it its communicator: qoc_set_time_comm), or -1: all
                                 * ranks emulated inside this one engine on one GPU (how the decomposition is tested) */
    int32_t gradient;           /* 0: the reference's first-order GRAPE gradient dK_t/du_k ~ H_k' K_t (the default); 1: the exact gradient -- the
                                 * derivative of the slice propagators the engine computes, Taylor truncation and squarings included, so that
                                 * value and gradient belong to the same function (what a line search assumes; it matters for few, long
                                 * slices).  Costates, regularisers, chain rule, Adam tail and stop rule are unchanged.  Runs on the generic
                                 * path (AUTO resolves to it); QOC_ERR_INVALID with any other explicit path or time_shards > 0, and for
                                 * taylor_terms > 60 or scaling > 12 (csrc/qoc_exact_grad.h) */
    int32_t reserved[2];
} qoc_config;

/* Adam loop hyper-parameters == Convergence (core/convergence.py:16-49). */
typedef struct qoc_adam_params {
    double rate;                /* convergence['rate']                 default 0.01  */
    double learning_rate_decay; /* convergence['learning_rate_decay']  default 2500   */
    double conv_target;         /* convergence['conv_target']          default 1e-8   */
    double min_grad;            /* convergence['min_grad']             default 1e-25  */
    int32_t max_iterations;     /* convergence['max_iterations']       default 5000   */
    int32_t poll_every;         /* host checks the device-side done flags every this many iterations (>=1) */
} qoc_adam_params;

/* ---- lifetime ---------------------------------------------------------------------------------------------------
 * qoc_create replaces TensorflowState(sys_para).build_graph() + tf.Session init
 * (main_grape/grape.py:113-114, core/run_session.py:27-29): constants are copied to HBM once.
 *   Hs   [(k+1)][n][n] complex : -i*dt*H0, -i*dt*Hops[k]     (matrix_list[:k+1] un-embedded, system_parameters.py:197-204)
 *   U0   [n][n] complex        : initial unitary              (tensorflow_state.py:162); ignored in state transfer
 *   V    [n][m] complex        : initial vectors as columns   (tensorflow_state.py:150-156)
 *   W    [n][m] complex        : target vectors as columns, U_target*V in unitary mode (tensorflow_state.py:158-166)
 *   maxA [k]                   : ops_max_amp                  (tensorflow_state.py:178)
 *   one_minus_gauss [k][steps] : envelope constant            (tensorflow_state.py:146-147); may be NULL if !has_envelope
 *   forbidden_states [n_forbidden], forbidden_coeffs [n_forbidden] (regularization_functions.py:81); any length
 *   Vs   [n][n] complex        : sort_ev(v_c, dressed_id), NULL unless forbid_dressed
 */
int qoc_create(const qoc_config* cfg, const double* Hs, const double* U0, const double* V, const double* W,
               const double* maxA, const double* one_minus_gauss, const int32_t* forbidden_states,
               const double* forbidden_coeffs, const double* Vs, qoc_handle* out);
int qoc_destroy(qoc_handle h);

/* ---- robust GRAPE: one pulse per control set over a weighted ensemble of Hamiltonians (no counterpart in the reference) --------
 * Member e is the reference problem with drift H0 + sum_q offsets[e][q] P_q and controls amp_scales[e][j] H_j; it shares U0, V, W, maxA,
 * the regularisers and the control set's pulse.  Per control set:
 *   loss      = sum_e weights[e] loss_e         (the value the stop rule tests)
 *   reg_loss  = loss + sum_e weights[e] (forbidden levels + speed_up)_e + the pulse regularisers of the shared pulse (counted once)
 *   grad      = d reg_loss / d base             (the members' gradients, weighted: first-order GRAPE, or exact with qoc_config.gradient = 1)
 *   unitary_scale = sum_e weights[e] unitary_scale_e;  grad_squared = sum grad^2 / 2 of that gradient
 * With sum weights = 1 these are the weighted means of the members' own values.  The engine runs n_seeds x members trajectories of k + q
 * controls (trajectory (g, e) = g * members + e; a perturbation is a frozen control row) and one Adam variable per control set.
 * Every other entry point keeps its per-control-set shapes ([n_seeds] ...); qoc_get_final_unitary and qoc_get_inter_vecs return member 0
 * of each control set.  Not available: the workgroup-resident path, the latency mode of the MFMA path (variant 5), time sharding, and
 * k + q > 8 on the paths limited to 8 controls (QOC_ERR_INVALID); AUTO never resolves to them for an ensemble. */
typedef struct qoc_ensemble {
    int32_t members;            /* E >= 1 */
    int32_t n_perturb;          /* q >= 0 */
    const double* P;            /* [q][n][n] complex: -i*dt*P_q (may be NULL when q = 0) */
    const double* offsets;      /* [E][q] */
    const double* amp_scales;   /* [E][k] */
    const double* weights;      /* [E], >= 0, used as given (the Python layer normalises them to sum 1) */
} qoc_ensemble;
/* cfg describes ONE member with n_seeds control sets (k = the real controls); the remaining arguments are exactly qoc_create's. */
int qoc_create_ensemble(const qoc_config* cfg, const qoc_ensemble* ens, const double* Hs, const double* U0, const double* V,
                        const double* W, const double* maxA, const double* one_minus_gauss, const int32_t* forbidden_states,
                        const double* forbidden_coeffs, const double* Vs, qoc_handle* out);
/* Per-member values of the last evaluation: loss [n_seeds][E] and reg_state [n_seeds][E] (forbidden levels + speed_up); any pointer may
 * be NULL.  QOC_ERR_STATE on an engine made by qoc_create. */
int qoc_get_member_scalars(qoc_handle h, double* loss, double* reg_state);
/* Every member's final unitary of the last evaluation: [n_seeds][E][n][n] complex (unitary mode only). */
int qoc_get_member_final_unitary(qoc_handle h, double* Uf);
/* The gradient array of the TRAJECTORIES as the backward kernels of the last evaluation left it, before the member reduction:
 * [n_seeds * E][kt + q][steps], dJ_e / du of every control row of every member (first order, or exact).  On the engines of
 * qoc_create_sparse_fleet the q frozen perturbation rows are cleared at creation and never written, so they read as exact zeros; what the dense
 * paths leave in those rows is not specified (no reduction reads them).  On a mapped engine the first kt rows are dJ / dc of the operators.
 * QOC_ERR_STATE on an engine that is no ensemble engine, or before the first evaluation. */
int qoc_get_trajectory_gradient(qoc_handle h, double* dLdu);

/* ---- risk-sensitive robust GRAPE: the soft worst case over the members in place of their weighted mean (no counterpart in the reference) ----
 * With beta > 0, the member costs c_e = loss_e + (forbidden levels + speed_up)_e and c_max their maximum, per control set:
 *   J        = c_max + log1p(sum_e weights[e] expm1(beta (c_e - c_max))) / beta     (members summed in the order 0 .. E-1)
 *   pi_e     = weights[e] exp(beta (c_e - c_max)) / (1 + that sum)                  = dJ / dc_e, the tilted weights
 *   grad     : the members' gradients weighted by pi_e in place of weights[e]
 *   reg_state = sum_e pi_e (forbidden levels + speed_up)_e;  loss = J - reg_state  (the value the stop rule tests: J itself without state
 *   regularisers);  reg_loss = J + the pulse regularisers;  unitary_scale stays the weights' mean.
 * With sum weights = 1, mean <= J <= max; beta = 0 (the default) is the weighted mean of qoc_create_ensemble, bit for bit, and beta -> infinity
 * the hard worst case (exp underflows to 0 on every member but the worst).  Valid on engines made by qoc_create_ensemble, qoc_create_shaped or qoc_create_mapped
 * (QOC_ERR_STATE on any other); beta negative, NaN or infinite: QOC_ERR_INVALID.  May be called between evaluations (annealing): it waits for
 * the enqueued work and holds from the next evaluation.  The first call with beta > 0 allocates the [n_seeds][E] weights. */
int qoc_set_risk(qoc_handle h, double beta);
/* pi_e of the last evaluation, [n_seeds][E]; the weights themselves at beta = 0 (and before the first evaluation under a risk).  A control
 * set that a loop has finished keeps the weights of its last evaluation.  QOC_ERR_STATE on a non-ensemble engine. */
int qoc_get_member_weights(qoc_handle h, double* pi);

/* ---- transfer-function GRAPE: the variable is the AWG's samples, the pulse a known linear response of them (no counterpart in the
 * reference, whose dwdt / bandpass / envelope penalties shrink what a line will not pass but do not model what it does) ----------------
 * T is a real steps x n_samples matrix (zero-order hold, interpolation, a filter or line response).  Per control set, with the variable
 * theta [k][P]:  w_s = sin(theta), the samples c = maxA_j w_s;  w_f[j][t] = sum_p T[t][p] w_s[j][p];  u_f = maxA_j w_f is the pulse
 * every trajectory runs on (member e of an ensemble: amp_scales[e][j] u_f).
 *   loss, unitary_scale, forbidden levels, speed_up : those of the steps-slice problem on u_f (coefficients divided by steps)
 *   amplitude, dwdt, d2wdt2, bandpass               : act on the SAMPLES, as the reference's terms with steps := P and
 *                                                     dt := total_time / P (coefficients divided by P; band indices from band * total_time)
 *   envelope                                        : rejected (its constant is defined per time slice)
 *   grad = d reg_loss / d theta                     : T^T applied to the members' weighted gradients, then the sample view's chain rule
 * qoc_set_base, qoc_get_base, qoc_eval's grad, qoc_get_uks and qoc_get_uks_evaluated are [n_seeds][k][P] on such an engine;
 * qoc_get_final_unitary and qoc_get_inter_vecs keep their steps shapes.  ens may be NULL: one nominal member.  The exclusions are the
 * ensemble's.  QOC_ERR_INVALID: n_samples < 1, a non-finite T, an all-zero column of T (a sample that never reaches the pulse),
 * has_envelope. */
typedef struct qoc_transfer {
    int32_t n_samples;          /* P >= 1 */
    const double* T;            /* [steps][n_samples] */
} qoc_transfer;
int qoc_create_shaped(const qoc_config* cfg, const qoc_ensemble* ens, const qoc_transfer* transfer, const double* Hs, const double* U0,
                      const double* V, const double* W, const double* maxA, const double* one_minus_gauss,
                      const int32_t* forbidden_states, const double* forbidden_coeffs, const double* Vs, qoc_handle* out);
/* u_f of the last evaluation, [n_seeds][k][steps] (the nominal pulse, before any member's amplitude scale).  QOC_ERR_STATE on an engine
 * not made by qoc_create_shaped. */
int qoc_get_pulse(qoc_handle h, double* u);

/* ---- control maps: the coefficients of the Hamiltonian as functions of the pulses (no counterpart in the reference, whose model is
 * H(t) = H0 + sum_k u_k(t) H_k: each pulse multiplies exactly one operator, linearly) ---------------------------------------------------------
 * For control set g and member e, v_j[t] is the pulse the member runs on without a map: amp_scales[e][j] maxA_j sin(base_g[j][t]), or the
 * filtered u_f of a transfer function, j < k = cfg->k.  The trajectory's coefficient of operator i = 1 .. r is
 *   c_i[t] = fixed[i][t] + sum_{j < k} mix[i][j][t] p_ij(v_j[t]),      p_ij(x) = sum_{d = 1 .. D} poly[i][j][d] x^d
 * and H(t) = H0 + sum_i c_i(t) G_i plus the member's frozen perturbation rows.  This covers crosstalk (a mixing matrix), carriers and frames (a
 * mixing matrix per slice), fixed drives and time-dependent drifts (fixed), and a nonlinear response of each line (poly); r need not equal k.
 *   grad: dJ/dv_j[t] = sum_i dJ/dc_i[t] mix[i][j][t] p_ij'(v_j[t]), with dJ/dc the trajectories' gradient (first order, or exact with
 *   qoc_config.gradient = 1), then the members' and the line's reduction and the tail as on every ensemble engine.
 * The variable, maxA, the pulse regularisers, qoc_get_uks, qoc_get_pulse and both optimiser loops stay on the k pulses; loss, unitary_scale and the
 * state regularisers are the trajectories'.  ens and transfer may each be NULL: one nominal member, no line.  Everything that works on an ensemble
 * engine works here (qoc_set_risk, the member read-backs, gradient = 1, qoc_run_adam, qoc_run_lbfgs); AUTO plans as for an ensemble whose
 * trajectories have r + q controls; qoc_plan_describe appends terms=r degree=D.  The identity map (r = k, D = 1, poly = I, no mix, no fixed)
 * computes the values of the same engine without a map, bit for bit.
 * QOC_ERR_INVALID, with the cause named and before any device is touched: a NULL map or poly; n_terms outside 1 .. 64; degree outside 1 .. 8; a
 * non-finite entry; a pulse that reaches no operator (poly[i][j][:] or mix[i][j][:] zero for every i); and the exclusions of qoc_create_ensemble /
 * qoc_create_shaped, with r + q in place of k + q on the paths limited to 8 controls. */
typedef struct qoc_control_map {
    int32_t n_terms;        /* r >= 1: Hs holds H0', G_1' .. G_r' (r + 1 operators, -i dt G_i) */
    int32_t degree;         /* D, 1 .. 8 */
    const double* poly;     /* [r][k][D]: alpha, powers 1 .. D */
    const double* mix;      /* [r][k][steps] or NULL (ones) */
    const double* fixed;    /* [r][steps] or NULL (zeros) */
} qoc_control_map;
/* cfg->k is the number of pulses; after map come exactly qoc_create_shaped's remaining arguments (Hs with r + 1 operators). */
int qoc_create_mapped(const qoc_config* cfg, const qoc_ensemble* ens, const qoc_transfer* transfer, const qoc_control_map* map,
                      const double* Hs, const double* U0, const double* V, const double* W, const double* maxA, const double* one_minus_gauss,
                      const int32_t* forbidden_states, const double* forbidden_coeffs, const double* Vs, qoc_handle* out);
/* c of member 0 of every control set at the last evaluation, [n_seeds][r][steps].  QOC_ERR_STATE on an engine not made by qoc_create_mapped. */
int qoc_get_coefficients(qoc_handle h, double* c);

/* ---- device fleets: one pulse per device, for F devices that differ in their member tables (no counterpart in the reference) ------------------
 * Device f is an ensemble of E members: member e has the drift H0 + sum_q offsets[f][e][q] P_q and the controls amp_scales[f][e][j] H_j.  The
 * devices share P, the weights, the risk, U0, V, W, maxA, the regularisers, the line and the control map.  cfg->n_seeds = F R control sets,
 * device-major: control set g belongs to device g / R and is its restart g % R.  Per control set every quantity -- loss, reg_loss, grad,
 * unitary_scale, the risk objective and its tilted weights, the stop rule -- is what qoc_create_ensemble, qoc_create_shaped or qoc_create_mapped
 * (whichever transfer and map select) defines for an ensemble with that device's rows; nothing couples control sets.  ens supplies members,
 * n_perturb, P and weights (its offsets and amp_scales are not read); ens NULL: one member per device, no perturbation.  Every read-back keeps
 * its [n_seeds] shape, the member read-backs and qoc_set_risk work as on an ensemble, and qoc_plan_describe appends devices=F.  AUTO plans as
 * for n_seeds x E trajectories.  A fleet of one device computes the values of the ensemble engine with the same rows, bit for bit.
 * QOC_ERR_INVALID, with the cause named and before any device is touched: a NULL fleet or amp_scales; NULL offsets with n_perturb > 0;
 * devices < 1; n_seeds no multiple of devices; a non-finite entry; and every exclusion of the ensemble's entry points. */
typedef struct qoc_fleet {
    int32_t devices;            /* F >= 1; cfg->n_seeds must be a multiple of it */
    const double* offsets;      /* [F][E][q] (may be NULL when q = 0) */
    const double* amp_scales;   /* [F][E][k] */
} qoc_fleet;
/* transfer and map may each be NULL; after map come exactly qoc_create_mapped's remaining arguments. */
int qoc_create_fleet(const qoc_config* cfg, const qoc_ensemble* ens, const qoc_fleet* fleet, const qoc_transfer* transfer,
                     const qoc_control_map* map, const double* Hs, const double* U0, const double* V, const double* W, const double* maxA,
                     const double* one_minus_gauss, const int32_t* forbidden_states, const double* forbidden_coeffs, const double* Vs,
                     qoc_handle* out);

/* ---- open-system GRAPE: the pulse is scored and optimised under a Lindblad master equation (no counterpart in the reference, whose graph
 * propagates state vectors) ----------------------------------------------------------------------------------------------------------------
 * Collapse operators C_j are n x n and carry the square root of their rates; the caller passes D_j = sqrt(dt) C_j.  With H' = -i dt H as in Hs:
 *   A_t = H0' + sum_k u_k[t] H_k' - 1/2 sum_j D_j^dagger D_j,   L_t(X) = A_t X + X A_t^dagger + sum_j D_j X D_j^dagger
 * Slice map: N = 2^scaling sub-steps, each X <- sum_{j = 0 .. taylor_terms} (L_t / N)^j X / j! (terms as a chain, summed in ascending j).  The
 * convention is the SAME in unitary and state-transfer mode: degree taylor_terms and 2^scaling sub-steps in both -- not the closed engine's degree
 * taylor_terms - 1 without squarings in state transfer.
 * The operators rho_ij(0) = psi_i psi_j^dagger of the m start vectors (U0 V in unitary mode, V in state transfer) are propagated and scored against
 * sigma_ij = w_i w_j^dagger (columns of W):
 *   loss          = 1 - (1 / m^2) sum_ij Re Tr(sigma_ij^dagger rho_ij(T))   (with n_collapse = 0: the closed engine's loss exactly; the relative
 *                                                                            phases of a gate are scored without a process-tomography basis)
 *   unitary_scale = (1 / m) sum_i Re Tr rho_ii(T)                           (1 for a trace-preserving map);  the state regulariser is 0
 *   grad          : first order as the reference's -- Lambda_ij(T) = -sigma_ij / m^2 carried back by the adjoint slice map,
 *                   dL/du[k, t] = sum_ij Re <Lambda_ij(t+1), H_k' rho_ij(t+1) + rho_ij(t+1) H_k'^dagger>; pulse regularisers, chain rule, Adam tail and
 *                   stop rule as on every engine, so qoc_eval, qoc_adam_step, qoc_iterate, qoc_run_adam, qoc_get_scalars, qoc_get_uks* and
 *                   qoc_set_base / qoc_get_base work as they are
 * Accepted: n_collapse = 0 (the closed limit), cfg.path AUTO or QOC_PATH_LINDBLAD, both modes, any n_seeds.  QOC_ERR_INVALID, before any device is
 * touched: forbidden levels, speed_up, forbid_dressed; gradient = 1; time_shards > 0; any other explicit path; n > 32, n_collapse > 8, m > n or
 * (n_collapse + 4) n (n | 1) 16 bytes > 159 KiB of LDS; taylor_terms < 1 or > 60; scaling > 12.  qoc_get_final_unitary, qoc_get_inter_vecs and the
 * member and pulse read-backs return QOC_ERR_STATE on such an engine; the two read-backs below return it on every other engine.
 * cfg.path = QOC_PATH_LINDBLAD_TILED (this entry point and the two below; never chosen by AUTO) lifts the size limits to 1 <= n <= 128 with any
 * n_collapse <= 8 and no LDS rule: the same mathematics on 16 x 16 tiles in global scratch, 5 NP^2 16 bytes per (control set, pair), NP = 16 ceil(n / 16);
 * QOC_ERR_NOMEM when that scratch cannot be allocated.  Everything else above holds as it stands. */
typedef struct qoc_open {
    int32_t n_collapse;         /* c >= 0 */
    const double* C;            /* [c][n][n] complex: sqrt(dt) C_j; NULL when c = 0 */
} qoc_open;
int qoc_create_open(const qoc_config* cfg, const qoc_open* open, const double* Hs, const double* U0, const double* V, const double* W,
                    const double* maxA, const double* one_minus_gauss, qoc_handle* out);
/* rho_ij(T) of the last evaluation, [n_seeds][m][m][n][n] complex: the pairs i > j mirrored from rho_ji (rho_ij = rho_ji^dagger) */
int qoc_get_final_density(qoc_handle h, double* rho);
/* Re rho_ii(tau)[l][l] of the last evaluation, [n_seeds][steps+1][n][m] (tau = 0 is the start): the populations a closed run derives from inter_vecs */
int qoc_get_populations(qoc_handle h, double* pop);

/* ---- open-system ensembles and fleets: every member with its own decay rates ----------------------------------------------------------------
 * A member of an ensemble, or of a device of a fleet, is a Hamiltonian AND its decay: member e of device f is the open problem above with the drift
 * H0 + sum_q offsets[f][e][q] P_q, the controls amp_scales[f][e][j] H_j and the collapse operators sqrt(rate_scales[f][e][j]) C_j (a scale of 0
 * switches the channel off for that member).  Per member everything is what qoc_create_open defines (the slice map with taylor_terms and 2^scaling
 * sub-steps in both modes, the pairs i <= j, loss, unitary_scale, a zero state regulariser, the first-order gradient); per control set everything is
 * what qoc_create_ensemble, qoc_create_shaped, qoc_create_mapped or qoc_create_fleet (whichever ens, fleet, transfer and map select) defines over
 * those members: the weighted mean, the soft worst case of qoc_set_risk, the line, the map's chain rule, the device g / R, the stop rule, Adam and
 * L-BFGS.  ens, fleet, transfer and map may each be NULL with the meaning they have in qoc_create_fleet; fleet NULL: one block of rows for every
 * control set; all four NULL: one nominal member, and with scales of 1 the values of qoc_create_open, bit for bit.  A fleet of one device computes
 * the values of the ensemble with its rows, bit for bit.
 * qoc_set_risk, qoc_get_member_scalars, qoc_get_member_weights, qoc_get_pulse (with a line), qoc_get_coefficients (with a map) and every loop work as
 * on any ensemble engine; qoc_get_final_density and qoc_get_populations return member 0 of each control set; qoc_get_final_unitary and
 * qoc_get_inter_vecs stay QOC_ERR_STATE.  qoc_plan_describe: the open engine's line with what the ensemble entry points append.
 * QOC_ERR_INVALID, with the cause named and before any device is touched: everything qoc_create_open refuses, everything the four ensemble entry
 * points refuse about their own tables, and a negative or non-finite rate scale. */
typedef struct qoc_decay {
    int32_t n_collapse;          /* c, 0 .. 8 */
    const double* C;             /* [c][n][n] complex: sqrt(dt) C_j at scale 1; NULL when c = 0 */
    const double* rate_scales;   /* [F][E][c], finite, >= 0; NULL: ones (F = fleet->devices, or 1) */
} qoc_decay;
/* after map come exactly qoc_create_open's remaining arguments */
int qoc_create_open_fleet(const qoc_config* cfg, const qoc_decay* decay, const qoc_ensemble* ens, const qoc_fleet* fleet,
                          const qoc_transfer* transfer, const qoc_control_map* map, const double* Hs, const double* U0, const double* V,
                          const double* W, const double* maxA, const double* one_minus_gauss, qoc_handle* out);
/* rho_ij(T) of every member at the last evaluation, [n_seeds][E][m][m][n][n] complex.  QOC_ERR_STATE on every other engine. */
int qoc_get_member_final_density(qoc_handle h, double* rho);

/* ---- open-system running costs: penalties on expectation values along the pulse (the reference's forbidden-level regulariser is the special case
 * of a projector on a closed system, regularization_functions.py:81-85) -----------------------------------------------------------------------
 * Per trajectory (a control set, or a member of one), with L observables O_l (n x n complex), coefficients a_l and powers p_l in {1, 2}:
 *   x_l,i(tau) = Re sum_ac conj(O_l[a][c]) rho_ii(tau)[a][c]                       (= Re Tr(O_l rho_ii(tau)) for a Hermitian O_l)
 *   R          = sum_l (a_l / steps) sum_{tau = 0 .. steps} sum_{i < m} x_l,i(tau)^p_l / p_l
 * R is the trajectory's state regulariser: reg_loss = loss + R + the pulse regularisers, the stop rule reads loss as before, and on an ensemble,
 * line, map or fleet the members' R go where the closed engines' forbidden levels go (the weighted mean, the cost c_e of qoc_set_risk,
 * qoc_get_member_scalars).  O_l = |l><l| with p = 2 is the reference's forbidden level, O_l = v v^dagger its dressed form.
 *   grad : the costates of the diagonal pairs get a source per slice -- Lambda_ii(t+1) += sum_l (a_l / steps) x_l,i(t+1)^(p_l - 1) O_l, added after
 *          rho_ii(t+1) is loaded and before the slice's contraction, once per slice (not per sub-step); off-diagonal pairs are untouched.  First order
 *          in dt, as the engine's gradient is.
 *   tau = 0 : the start operators (from U0 V in unitary mode, V in state transfer) count in the value and, being independent of the pulse, not in the
 *          gradient -- the convention of qoc_get_populations.  (The reference's closed regulariser takes V itself at tau = 0: the closed-limit value
 *          equals it in state transfer and in unitary mode with U0 = I, and differs by that pulse-independent term otherwise.)
 * qoc_create_open_costs takes everything qoc_create_open_fleet takes, with the same meaning (all four of ens, fleet, transfer and map may be NULL);
 * with n_obs = 0 (costs may then be NULL) it computes qoc_create_open_fleet's values bit for bit; with n_obs > 0 qoc_plan_describe appends
 * running_costs=<L>.  Two evaluations are bit-identical.
 * QOC_ERR_INVALID, with the cause named and before any device is touched: everything qoc_create_open_fleet refuses (cfg.n_forbidden, has_speed_up and
 * forbid_dressed included: they keep their meaning); NULL arrays with n_obs > 0; n_obs outside 0 .. 16; a power other than 1 or 2; a non-finite entry
 * or coefficient. */
typedef struct qoc_running_costs {
    int32_t n_obs;               /* L, 0 .. 16 */
    const double* O;             /* [L][n][n] complex, row-major */
    const double* coeffs;        /* [L] finite; the engine divides by cfg->steps */
    const int32_t* powers;       /* [L] 1 or 2 */
} qoc_running_costs;
/* after map come exactly qoc_create_open's remaining arguments */
int qoc_create_open_costs(const qoc_config* cfg, const qoc_decay* decay, const qoc_running_costs* costs, const qoc_ensemble* ens,
                          const qoc_fleet* fleet, const qoc_transfer* transfer, const qoc_control_map* map, const double* Hs, const double* U0,
                          const double* V, const double* W, const double* maxA, const double* one_minus_gauss, qoc_handle* out);
/* x_l,i(tau) of the last evaluation, [n_seeds][steps+1][L][m] (tau = 0 is the start; member 0 of each control set).  QOC_ERR_STATE on every engine
 * without running costs. */
int qoc_get_expectations(qoc_handle h, double* x);

/* ---- sparse state transfer: the operators are never dense (the reference has sparse_H / sparse_U / sparse_K for systems built from Kronecker products
 * and switches them off under use_gpu, main_grape/grape.py:28-32) ----------------------------------------------------------------------------
 * The k + 1 operators -i dt H0, -i dt H_1 .. come as COO entries in any order; duplicates of a position are summed, explicit zeros are kept.  The
 * engine stores each in ELLPACK with a width of its own (the largest number of entries in one of its rows) and never forms an n x n array, on the
 * host or on the device: memory is O(sum_j n W_j + n_seeds steps n m), so n = 2^14 and beyond fit where one dense operator would not.
 * The mathematics is the state-transfer branch of every other engine (matvecexp_op: psi_{t+1} = sum_{j < taylor_terms} B_t^j psi_t / j!, costates with
 * -B_t, first-order gradient), with loss, unitary_scale, bare forbidden levels, speed_up, every pulse regulariser, the Adam tail, the L-BFGS step and
 * the stop rule unchanged, so every entry point below works as on any engine; qoc_get_final_unitary returns QOC_ERR_STATE as for state transfer elsewhere.
 * Operators need not be Hermitian.  Two evaluations are bit-identical, and so are the two vector homes.
 * QOC_ERR_INVALID, with the cause named and before any device is touched: unitary mode; forbid_dressed; gradient = 1; time_shards > 0; an explicit path
 * other than AUTO or QOC_PATH_SPARSE; taylor_terms < 1 or > 60; m < 1; an index outside 0 .. n-1; a non-finite value; n * W_j (or n * m) past int32;
 * vector_home outside 0 .. 2, or 1 where the vectors do not fit.  Device memory that does not fit: QOC_ERR_NOMEM. */
typedef struct qoc_sparse {
    const int64_t* indptr;      /* [k+2] operator j owns entries indptr[j] .. indptr[j+1] of the three arrays below */
    const int32_t* row;
    const int32_t* col;
    const double* val;          /* complex (re, im): -i dt H_j */
    int32_t vector_home;        /* where the two vectors of a sweep's Taylor chain live: 0 auto (LDS while 2 n 16 B <= 159 KiB, i.e. n <= 5088),
                                 * 1 LDS (QOC_ERR_INVALID if it does not fit), 2 global scratch */
} qoc_sparse;
int qoc_create_sparse(const qoc_config* cfg, const qoc_sparse* ops, const double* V, const double* W, const double* maxA,
                      const double* one_minus_gauss, const int32_t* forbidden_states, const double* forbidden_coeffs, qoc_handle* out);

/* ---- sparse ensembles, fleets, lines and maps: the ensemble entry points on sparse operators ------------------------------------------------
 * ens, fleet, transfer and map may each be NULL with the meaning they have in qoc_create_fleet; per control set every quantity is what those entry
 * points define over the members, per member everything is what qoc_create_sparse defines.  ops holds kt + 1 + q operators in the order
 * [H0, H_1 .. H_kt, P_1 .. P_q] with kt = map ? map->n_terms : cfg->k and q = ens->n_perturb (indptr has kt + q + 2 entries): the perturbation
 * operators are the last q of ops and ens->P must be NULL.  All four NULL: one nominal member, and with row_layout = 1 the values of
 * qoc_create_sparse, bit for bit.
 * plan (may be NULL: all auto) selects how a sweep walks the operators of a row:
 *   1 per operator   the kernels of qoc_create_sparse: one ELLPACK block per operator, kt + q + 1 passes per Taylor term
 *   2 merged         the stored entries of all operators of a row in ONE list (operator 0 first, columns ascending inside an operator, padding
 *                    dropped), each slot a column and an operator index packed as col | op << 24; the slice's coefficients come from a table in
 *                    LDS.  The arithmetic order is the per-operator kernels', so both layouts compute the same numbers (equal under ==; the sign
 *                    of a zero may differ).  At most 255 operators and n < 2^24
 *   0 auto           merged for n >= 1024 with 12 or more operators, where it was measured ahead (QOC_SP_MERGED_AUTO in csrc/qoc_sparse.h,
 *                    profiles/sparse_ensemble.txt), per operator everywhere else and where 2 cannot run
 * The gradient kernel reads each control's own ELLPACK block in both layouts and forms no gradient for the frozen perturbation rows.
 * The vectors of a merged sweep live in LDS while 2 n 16 B + the table (8 B per operator, rounded up to 16 B) <= 159 KiB.
 * qoc_plan_describe: the sparse engine's line with rows=<per_operator|merged> merged_width=<longest merged row, 0 per operator> and what the ensemble
 * entry points append.  The ensemble getters work as on a dense ensemble engine; the final-unitary getters keep their state-transfer refusal.
 * QOC_ERR_INVALID, with the cause named and before any device is touched: everything qoc_create_sparse refuses; everything the four ensemble entry
 * points refuse about member counts, weights, tables, devices, the line and the map; a non-NULL ens->P; row_layout outside 0 .. 2; row_layout = 2
 * with more than 255 operators or n >= 2^24. */
typedef struct qoc_sparse_plan {
    int32_t row_layout;         /* 0 auto, 1 per operator, 2 merged */
} qoc_sparse_plan;
int qoc_create_sparse_fleet(const qoc_config* cfg, const qoc_sparse* ops, const qoc_sparse_plan* plan, const qoc_ensemble* ens, const qoc_fleet* fleet,
                            const qoc_transfer* transfer, const qoc_control_map* map, const double* V, const double* W, const double* maxA,
                            const double* one_minus_gauss, const int32_t* forbidden_states, const double* forbidden_coeffs, qoc_handle* out);

/* ---- noise traces: ensemble members with time-dependent perturbations -------------------------------------------------------------------------
 * Every member table above holds errors that are constant over the pulse (offsets), and collapse operators hold white noise; a trace table is what
 * lies between: sampled noise trajectories (1/f-like flux noise, a detuning that drifts during the gate, a switching fluctuator), one per member
 * and perturbation.  With a table set, frozen row q' of member e of device f has at slice t the value
 *     offsets[f][e][q'] + traces[f][e][q'][t]
 * (one fp64 add, formed where the row is written), and everything else is what the engine defines for that control row: the trajectories' k + q
 * (with a map: r + q) controls on every route -- dense, open (the slice's generator reads every row per slice) and sparse (both row layouts) --,
 * the member reduction, qoc_set_risk, lines, maps, fleets, gradient = 1, both loops and the stop rule.  The objective is the sample average (or
 * soft worst case) over the fixed set of traces.  taylor_terms and scaling stay the caller's: choose them for the largest |offsets + traces[t]|.
 * traces: [F][E][q][steps] with F = the fleet's devices, 1 without a fleet; NULL removes the table.  Without a table an engine launches exactly the
 * kernels it launched before this entry point existed; while one is set qoc_plan_describe appends traces=1.  Two evaluations are bit-identical; an
 * all-zero table computes the values of no table, and offsets 0 with constant traces c the values of offsets c (equal under ==).
 * Valid on every engine with a member table and q >= 1 (qoc_create_ensemble, _shaped, _mapped, _fleet, _open_fleet, _open_costs, _sparse_fleet).
 * QOC_ERR_STATE, with the cause named: an engine without a member table (qoc_create, qoc_create_open, qoc_create_sparse); q = 0.
 * QOC_ERR_INVALID: a non-finite entry.  QOC_ERR_NOMEM: the device copy does not fit.
 * Timing as for qoc_set_risk: it may be called between evaluations or bursts of qoc_iterate / qoc_iterate_lbfgs (fresh draws every N iterations); it
 * waits for the enqueued work and holds from the next evaluation.  The first call with a table allocates the device copy, later calls overwrite it.
 * The setter resets NOTHING: Adam moments, the L-BFGS history and accepted point, iteration counters and done flags stay as they are.  A new table is
 * a new objective: a caller who resamples under L-BFGS owns the consequences (curvature pairs and the Armijo reference value belong to the old
 * one), and a control set that a loop has finished stays finished. */
int qoc_set_traces(qoc_handle h, const double* traces);

/* ---- the trainable variable -------------------------------------------------------------------------------------
 * ops_weight_base [n_seeds][k][steps]  (tensorflow_state.py:174; ops_weight_base.assign, run_session.py:121).
 * qoc_set_base also resets the Adam slots and the per-seed iteration counters / done flags. */
int qoc_set_base(qoc_handle h, const double* base);
int qoc_get_base(qoc_handle h, double* base);

/* ---- one evaluation == session.run([grad_pack, loss, reg_loss, unitary_scale, grad_squared])
 * (run_session.py:53-54 and get_error :119-127).  Arrays are [n_seeds]; grad is [n_seeds][k][steps] =
 * d reg_loss / d ops_weight_base with the reference's first-order GRAPE gradient (tensorflow_state.py:49-65,
 * 100-133) -- or, on an engine created with qoc_config.gradient = 1, with the exact derivative of the computed slice
 * propagators in its place; any output pointer may be NULL. */
int qoc_eval(qoc_handle h, double* loss, double* reg_loss, double* grad_squared, double* unitary_scale,
             double* grad);

/* ---- one optimizer application == session.run([optimizer], {learning_rate: lr}) (run_session.py:66-69):
 * TF1 Adam (beta1 .9, beta2 .999, eps 1e-8 outside the bias correction) on the gradient of the last evaluation
 * (the reference recomputes it at the same parameters, which is numerically the same).  lr is [n_seeds]. */
int qoc_adam_step(qoc_handle h, const double* lr);

/* ---- device-resident optimisation loop == run_session.start_adam_optimizer (run_session.py:47-69), per seed:
 * evaluate; stop if loss < conv_target or grad_squared < min_grad or iterations >= max_iterations; otherwise
 * iterations += 1, lr = rate*exp(-iterations/decay), Adam step.  Stop decisions are taken on the device per seed
 * (finished seeds freeze); the host only polls.  iterations_out is [n_seeds] (may be NULL). */
int qoc_run_adam(qoc_handle h, const qoc_adam_params* p, int32_t* iterations_out);

/* Enqueue exactly `iters` loop iterations (same per-seed semantics as qoc_run_adam) without any host
 * synchronisation; used by bench.py between two qoc_sync() calls. */
int qoc_iterate(qoc_handle h, const qoc_adam_params* p, int32_t iters);
int qoc_sync(qoc_handle h);

/* ---- device-resident L-BFGS loop (no counterpart in the reference, whose L-BFGS-B is scipy's, one host round trip per evaluation) ------------
 * One loop iteration is the evaluation of qoc_eval followed by one step kernel (csrc/qoc_lbfgs.h); the objective is reg_loss, the variable base.
 * Every control set keeps its own history of `history` curvature pairs, direction, step length and flags, so n_seeds restarts are n_seeds
 * independent quasi-Newton runs.  Per control set and evaluation (f, g = reg_loss and its gradient at x = base):
 *   the evaluation of a restored point ends the set;  loss < conv_target or grad_squared < min_grad ends it where it stands;
 *   acceptable = first evaluation, or f finite and f <= f_acc + c1 alpha g_acc.p (Armijo);
 *   iterations >= max_iterations: done if acceptable, else base = x_acc and one more evaluation there (a set ends with its last evaluation
 *     at the point it returns, after at most max_iterations + 2 evaluations);  otherwise iterations += 1 and
 *   accept: the pair (x - x_acc, g - g_acc) enters the history if s.y > 1e-10 y.y; p = -H g by the L-BFGS recursion with H0 = (s.y / y.y) I of the
 *     newest pair (empty history, or g.p >= 0 which also clears it: p = -g / |g|); alpha = 1; base = x + p;
 *   reject: after max_ls rejected trials the history is cleared and the search restarts along -g_acc / |g_acc| with alpha = 1 (a search that
 *     was steepest descent already: base = x_acc, one more evaluation, done); otherwise alpha *= shrink, base = x_acc + alpha p.
 * Backtracking Armijo, no bounds, no interpolation.  The state ((2 history + 3) vectors of the variable's size per control set)
 * is allocated by the first call: QOC_ERR_NOMEM if it does not fit (a later call with a longer history takes one more block, for 16 pairs; the
 * engine keeps both until qoc_destroy).  qoc_set_base resets it as it resets the Adam slots; a call with another
 * `history` resets it too.  QOC_ERR_INVALID (the message starts with the call's name): null params, history outside 1 .. 16, c1 or shrink
 * outside (0, 1), max_ls < 1, a time-sharded engine.  Works on every other engine: ensembles, transfer functions, the exact gradient, open
 * systems.  Finished control sets keep being evaluated at their final point, so every read-back belongs to it. */
typedef struct qoc_lbfgs_params {
    double conv_target, min_grad;      /* as qoc_adam_params */
    double c1;                         /* Armijo constant, default 1e-4 */
    double shrink;                     /* step factor on a rejected trial, default 0.5, in (0, 1) */
    int32_t max_iterations;            /* as qoc_adam_params: bounds the evaluations (see the stop rule) */
    int32_t history;                   /* M pairs kept, 1 .. 16, default 8 */
    int32_t max_ls;                    /* rejected trials before the direction is reset, default 20 */
    int32_t poll_every;
} qoc_lbfgs_params;
int qoc_iterate_lbfgs(qoc_handle h, const qoc_lbfgs_params* p, int32_t iters);      /* no host sync, like qoc_iterate */
int qoc_run_lbfgs(qoc_handle h, const qoc_lbfgs_params* p, int32_t* iterations_out); /* polls done flags, like qoc_run_adam */

/* Last evaluation's per-seed scalars [n_seeds] each (any pointer may be NULL). */
int qoc_get_scalars(qoc_handle h, double* loss, double* reg_loss, double* grad_squared, double* unitary_scale,
                    int32_t* iterations, int32_t* done);

/* ---- read-back == Analysis (core/analysis.py:18-41) and run_session.Get_uks (run_session.py:112-117) ----------
 * uks   [n_seeds][k][steps]          : maxA[k] * sin(base) of the current variable
 * Uf    [n_seeds][n][n] complex      : RtoCMat(final_state) of the last evaluation (unitary mode only)
 * inter [n_seeds][steps+1][n][m] cplx: inter_vecs (tau = 0 is the initial vectors) of the last evaluation */
int qoc_get_uks(qoc_handle h, double* uks);
/* uks the LAST EVALUATION ran on (inside the Adam loop the variable has already moved one step further; the reference
 * logs loss, final_state and uks of the same evaluation, run_session.py:75-91,130-138). */
int qoc_get_uks_evaluated(qoc_handle h, double* uks);
int qoc_get_final_unitary(qoc_handle h, double* Uf);
int qoc_get_inter_vecs(qoc_handle h, double* inter);

/* ---- measurement hooks (bench.py) -------------------------------------------------------------------------------
 * With profiling enabled every launch of the dominant kernel is bracketed by hipEvents on the engine's stream.
 * qoc_profile_read returns the number of bracketed launches and their summed duration in milliseconds. */
int qoc_profile_enable(qoc_handle h, int32_t on);
int qoc_profile_read(qoc_handle h, const char** kernel_name, int64_t* launches, double* total_ms);
/* Elapsed milliseconds (hipEvents on the engine stream) around `iters` iterations, after a sync. */
int qoc_time_iterations(qoc_handle h, const qoc_adam_params* p, int32_t iters, double* elapsed_ms);

/* ---- multi-GPU: seed-parallel sharding, one process per GPU (the reference is single-device,
 * main_grape/grape.py:106-109, and optimises ONE control set per call, core/system_parameters.py:272-284) -------------
 * Restarts are independent, so the data path has no collective.  The only exchange is an all-gather of per-seed scalars
 * (final fidelities) over RCCL/xGMI and an optional broadcast of the winner's pulse.  librccl is opened at run time
 * (dlopen, from the ROCm tree of this library's HIP runtime; QOC_RCCL_LIBRARY overrides), so single-GPU use needs no RCCL.
 * The 128-byte id is created on rank 0 and handed to the other ranks by the launcher (any side channel; the Python host
 * uses a file rendezvous, quantum_optimal_control/parallel_seeds.py). */
typedef struct qoc_comm* qoc_comm_handle;
#define QOC_COMM_ID_BYTES 128
int qoc_comm_unique_id(void* id128);
/* The local preconditions of qoc_comm_create (librccl loadable, device index valid, a stream can be made on it), no collective:
 * every rank checks them and the ranks agree on the outcome BEFORE anybody enters ncclCommInitRank, which would otherwise
 * wait forever for a rank that failed earlier. */
int qoc_comm_probe(int32_t device);
int qoc_comm_create(const void* id128, int32_t world, int32_t rank, int32_t device, qoc_comm_handle* out);
int qoc_comm_destroy(qoc_comm_handle c);
int qoc_comm_world(qoc_comm_handle c);
int qoc_comm_rank(qoc_comm_handle c);
const char* qoc_comm_library(void);        /* path of the librccl in use ("" before the first communicator) */
/* All-gather of one per-seed scalar array of the engine, device to device on the ENGINE's stream (ordered behind the
 * iterations already enqueued, no host synchronisation before the collective).  which: 0 loss, 1 reg_loss,
 * 2 grad_squared, 3 unitary_scale.  width >= n_seeds on every rank (rows are zero padded).  out: [world][width] (host). */
int qoc_comm_all_gather_scalar(qoc_comm_handle c, qoc_handle h, int32_t which, int32_t width, double* out);
/* Host-buffer collectives on the communicator's own stream: recv is [world][count]. */
int qoc_comm_all_gather_f64(qoc_comm_handle c, const double* send, int32_t count, double* recv);
int qoc_comm_all_reduce_max_f64(qoc_comm_handle c, double* inout, int32_t count);
int qoc_comm_broadcast_f64(qoc_comm_handle c, double* buf, int64_t count, int32_t root);
int qoc_comm_barrier(qoc_comm_handle c);

/* Time-sharded engines (qoc_config.time_shards >= 1, time_rank >= 0): the communicator whose ranks hold the other time shards; world and
 * rank must equal time_shards / time_rank.  The engine's iterations then contain RCCL calls: every rank must enqueue the same iterations
 * (and qoc_get_inter_vecs is a collective too: each rank holds the time points of its own slices, the call sums them over the ranks).
 * Lifetime: the communicator must outlive the engine -- qoc_comm_destroy returns QOC_ERR_STATE while an engine still holds it; qoc_destroy
 * of the engine releases it. */
int qoc_set_time_comm(qoc_handle h, qoc_comm_handle c);

/* ---- introspection ---------------------------------------------------------------------------------------------*/
int qoc_path_in_use(qoc_handle h);        /* the QOC_PATH_* the engine resolved AUTO to */
int qoc_chunks_in_use(qoc_handle h);
/* One line of key=value pairs naming what AUTO resolved to (path, kernel family of the exponentials, chunk count, sweep kernels / route):
 * no counterpart in the reference (TensorFlow places its ops itself); the dispatch test tests/test_auto_plan.py reads it. */
int qoc_plan_describe(qoc_handle h, char* buf, int32_t len);
int qoc_device_count(void);
int qoc_device_info(int32_t device, char* name, int32_t name_len, int32_t* compute_units, int64_t* hbm_bytes);
/* hipDeviceCanAccessPeer(device, peer): 1 when `device` can address the memory of `peer` directly (xGMI / PCIe peer-to-peer), which is what RCCL's
 * device-to-device transports between two ranks of a node need; tools/multi_gpu_selftest.py prints the matrix.  The reference runs on one device
 * (main_grape/grape.py:106-109) and has no counterpart. */
int qoc_device_peer_access(int32_t device, int32_t peer, int32_t* can_access);
const char* qoc_last_error(void);
const char* qoc_version(void);

#ifdef __cplusplus
}
#endif
#endif /* QOC_H */
