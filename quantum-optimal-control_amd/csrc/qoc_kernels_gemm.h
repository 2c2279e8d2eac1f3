// qoc_kernels_gemm.h -- "GEMM path" (QOC_PATH_GEMM): any n, m <= 32, unitary mode and state transfer.  The one header the engine includes for it.
//
// Matrices are zero-padded to N = 32*ceil(n/32) and live in HBM/L2 as plain row-major complex128.  Time is cut into NC
// chunks of S = 2^L ~ sqrt(steps) slices so that every chain has NC + S sequential steps instead of `steps`:
//   * exponentials for all (seed, slice) pairs: k_gemm_expm_fused (N <= 64) or batched k_zgemm32 / k_zgemm_wg launches of the
//     Paterson-Stockmeyer polynomial + squarings;
//   * a pairwise product tree gives the chunk products (and, in unitary mode, final_state at the root);
//   * forward / backward: chunk boundaries sequentially, then all chunks swept in parallel;
//   * control gradients: products H_k' [Psi_0 ... Psi_t ...] with a dot-product epilogue against conj(Lambda).
// Three routes (QocGemmRoute, fixed by qoc_gemm_setup): "persistent" -- N <= 64, m <= 8, the thin chains as persistent VALU kernels;
// "stepwise" -- everything larger, one batched product launch per step; "direct" -- state transfer on Taylor mat-vec chains over the
// assembled generators, no propagators.  State transfer otherwise runs through the same propagators (anti-Hermitian generators).
// Reference semantics: core/tensorflow_state.py:25-46, 49-65, 77-133, 204-261.
//
// Kernels (and their argument structs), nothing else:
//   qoc_gemm_tiles.h      k_zgemm32, k_zgemm_wg (GemmArgs)
//   qoc_gemm_expm.h       k_gemm_expm_fused (ExpmCoef)
//   qoc_gemm_chains.h     k_gemm_chain_fwd, k_gemm_taylor_chain, k_gemm_scan_nodes (ChainArgs, ScanArgs); qoc_gemm_chain_dpp.h, qoc_gemm_chain_sq.h
//   qoc_gemm_glue.h       assembly, chain starts and boundaries, layouts, sources, gradient reductions
// Host:
//   qoc_gemm_setup.h      QocGemm, the route and its predicates, qoc_gemm_setup in steps (decision, arena, host images, clears, overlap streams)
//   qoc_gemm_launch.h     makers of GemmArgs, the launchers (one qoc_pick per template ladder), qoc_gemm_lds_opt_in
//   qoc_gemm_routes.h     qoc_gemm_expm / _forward / _backward: one function per route and phase
//   qoc_gemm_ts.h         time-sharded evaluation on the stepwise pieces (included by the engine after this header)
#pragma once
#include "qoc_gemm_routes.h"
