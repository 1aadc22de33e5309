// Internal host-side declarations (C++ linkage) shared between the translation units of libarcvae_hip.so.
// The C ABI -- flag bits, error codes, every extern "C" prototype -- is include/arcvae_hip.h, which common.h includes: nothing
// of it is re-declared here.
#pragma once
#include "common.h"

// internal (C++ linkage): grouped weight-gradient GEMMs, see gemm.hip
// allow_split: bit 0 = split-bf16 kernel, bit 1 = its 128-row tile, bit 2 = one bf16 product (throughput mode), bit 3 = three-piece
// tile GEMM, bit 4 (with bit 0 alone) = the LDS-staged quiet form of the split-bf16 kernel (ARCVAE_GEMM_QUIET)
int arcvae_gemm_tn_group_accum(int n, int M, int N, const int* K, const float* const* A, int lda,
                               const float* const* B, int ldb, float* const* C, int ldc, int allow_split,
                               float* const* colsum /* optional: colsum_i[M] += column sums of A_i */, hipStream_t stream);

// internal (C++ linkage): arcvae_gemm_f32 with a gap in one dimension, see gemm.hip.  gap_dim: 0 none, 1 M, 2 N, 3 K; M, N, K are the
// LOGICAL extents; tiles at or beyond gap_at (a multiple of 64, as is gap_len) address gap_len further on in the operands, the bias
// and C.  colsum (optional, TN form only): colsum[m] += column sums of A over K -- the split kernel's rider where that kernel runs.
int arcvae_gemm_f32_gap(int transA, int transB, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C,
                        int ldc, const float* bias, int flags, int gap_dim, int gap_at, int gap_len, float* colsum,
                        hipStream_t stream);

// internal (C++ linkage): throughput mode, weight gradients from octet-major bf16 operand copies, see gemm.hip
int arcvae_wgrad_octet_group(int n, int M, int N, const int* K, const void* const* A, const void* const* B,
                             float* const* C, int ldc, hipStream_t stream);

// internal (C++ linkage): weight gradients of the tiled three-piece sweeps from their operand planes, see gemm.hip
int arcvae_wgrad_planes_group(int n, int M, int N, int rows, const void* const* A, const int* tA0, const void* const* B,
                              const int* tB0, const int* nT, float* const* C, int ldc, float* const* colsum /* optional */,
                              hipStream_t stream);

// internal (C++ linkage): a forward-only decoder layer (GEMM + zero-state cell, no pre-activations kept), see gemm.hip
// three_gates: the forget gate's columns are not computed (the zero-state cell never reads them)
int arcvae_gemm_cell_zero(int M, int H, int K, const float* A, int lda, const float* W, int ldw, const float* bias,
                          float* Hout, int three_gates, hipStream_t stream);

// internal (C++ linkage): two skinny products in one launch, see gemm.hip
int arcvae_gemm_skinny_pair(int transB, const int* M, const int* N, const int* K, const float* const* A, const int* lda,
                            const float* const* B, const int* ldb, float* const* C, const int* ldc,
                            const float* const* bias, const int* flags, hipStream_t stream);

// internal (C++ linkage): the unclipped forms of arcvae_adam_step (clip.hip) on misc.hip's adam_kernel; arguments checked there
int arcvae_adam_step_plain(float* params, const float* grads, float* m, float* v, long n, const float* lr_dev, double beta1,
                           double beta2, double eps, const unsigned* guard_a, const unsigned* guard_b, const float* rowloss,
                           int B, float* stats, float* scalars, int Z, int T, hipStream_t stream);
