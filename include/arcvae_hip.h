/* arcvae_hip.h -- C ABI of libarcvae_hip.so: the MI355X (gfx950) kernels behind the SELFIES
 * AR-CVAE training path of Raiden-Makoto/MLX-VAE.
 *
 * The reference has no FFI boundary of its own (its only boundary is the
 * Python module API on top of the third-party `mlx` runtime), so this header IS the kernel
 * boundary a maintainer would bind: each entry point replaces the MLX graph that one reference
 * function builds, named in the comment above it (file:line under the reference tree).
 *
 * Conventions (all entry points):
 *   - return 0 on success, negative on error (ARCVAE_ERR_*); no exceptions cross the ABI;
 *   - no allocation, no ownership transfer: every buffer is caller-owned DEVICE memory,
 *     contiguous row-major float32 unless stated, parameter tensors 16-byte aligned;
 *   - asynchronous on `stream` (a hipStream_t passed as void*); safe under hipGraph capture
 *     (no sync, no malloc); re-entrant: no global mutable host state -- chunk indices, trace buffers and
 *     sync scratch are arguments; the only process-wide values are the ARCVAE_* tuning knobs of the environment (most
 *     are read once per process; the kernel-family selectors -- ARCVAE_STEP_TILE, ARCVAE_RING, ARCVAE_PERSIST*,
 *     ARCVAE_RS_* -- are read at every call, so a caller that changes them must drop its captured graphs);
 *   - `const float* const*` arguments are HOST arrays of device pointers (one per LSTM layer);
 *   - gradients are accumulated ("+="): zero the flat gradient buffer once per step;
 *   - float32 arithmetic throughout (the reference's dtype), contractions on the exact-f32
 *     MFMA forms; hidden_dim a multiple of 64 and <= 512, num_layers <= 8, 1 <= num_conditions <= 8,
 *     vocab_size <= 255 (anything else is ARCVAE_ERR_ARG, never a silent fallback).
 */
#ifndef ARCVAE_HIP_H
#define ARCVAE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARCVAE_OK 0
#define ARCVAE_ERR_ARG (-1)
#define ARCVAE_ERR_LAUNCH (-2)
#define ARCVAE_ERR_DEVICE (-3)

#define ARCVAE_GEMM_ACCUMULATE 1 /* C += ...                                   */
#define ARCVAE_GEMM_TANH 2       /* C = tanh(...)                              */
#define ARCVAE_GEMM_SPLITK 4     /* allow split-K with f32 atomics             */
#define ARCVAE_GEMM_NO_SKINNY 8
#define ARCVAE_GEMM_TILE64 16   /* force 64x64 tiles (tuning / tests) */
#define ARCVAE_GEMM_TILE128 32  /* force 128x128 tiles */
#define ARCVAE_GEMM_DTANH 64    /* C = (A.B) * (1 - T^2), T = `bias` read as an [M,ldc] matrix (tanh backward) */
#define ARCVAE_GEMM_TILE_WIDE 128 /* split-bf16 TN path: 128-row tile (no persistent sweep resident beside it) */
#define ARCVAE_GEMM_BF16 256      /* throughput mode: operands rounded to bf16 (RNE), f32 accumulate on v_mfma_f32_32x32x16_bf16;
                                   * NOT a parity path (SURVEY.md section 8(d) Config 2 "bf16-in/fp32-acc"); products with M <= 256
                                   * rows on the dependent chain keep the f32 skinny kernel */
#define ARCVAE_GEMM_SPLIT3 512    /* any layout: every f32 operand as three bf16 pieces (8+8+8 bits), the six products of weight
                                   * >= 2^-16 on v_mfma_f32_32x32x16_bf16, f32 accumulate -- the accuracy class of the exact-f32
                                   * kernels (a PARITY path) at 2.7x less matrix-pipe time; for GEMMs beside a persistent sweep */
#define ARCVAE_GEMM_QUIET 1024    /* TN "+=" with ARCVAE_GEMM_SPLITK: the split-bf16 arithmetic (three pieces, six products, f32
                                   * accumulate: a PARITY path) with 128 x 128 block tiles whose operands are staged once in LDS by
                                   * 16-byte LDS-DMA and shared by the block's waves -- a quarter of the bytes and far fewer load
                                   * instructions than the LDS-free split kernel: for GEMMs beside the bs-64 BPTT sweep.  Needs
                                   * M, N, lda, ldb multiples of 4 and 16-byte aligned A, B (ARCVAE_ERR_ARG otherwise) */
#define ARCVAE_LSTM_RETILE 1     /* arcvae_enc_lstm_backward flags bit 0: write the BPTT weight layouts first */
#define ARCVAE_LSTM_BF16 2        /* arcvae_enc_lstm_forward / _backward flags bit 1: throughput mode -- bf16 operand copies and
                                   * v_mfma_f32_16x16x32_bf16 products where the shape runs on the register-tiled step kernels
                                   * (the MFMA-bound regime, e.g. H512 L4 bs 512); gates, cell state and accumulators stay f32.
                                   * The k-chunk-major workspaces (hseq_t, dG_t, wt, wT) then hold bf16 in 32-wide chunks --
                                   * same pointers, half the bytes; forward and backward of a step must be given the same flag */
#define ARCVAE_LSTM_SPLIT3 4      /* arcvae_enc_lstm_forward / _backward flags bit 2 (what the engine passes on the PARITY path): where the
                                   * shape runs on the register-tiled step kernels every operand value is three bf16 pieces (hi + mid
                                   * + lo, 8 + 8 + 8 bits), six products on v_mfma_f32_16x16x32_bf16, f32 accumulate -- the accuracy
                                   * class of the exact-f32 kernels.  The operand workspaces (hseq_t, dG_t, wt, wT) then hold THREE
                                   * bf16 planes per value: 6 bytes instead of 4, i.e. 3/2 of the f32 sizes, and where the weight
                                   * gradients read those planes the rings keep all T time slots: size them with
                                   * arcvae_enc_lstm_ws_floats and pass the capacities to every call (ws_floats) */
#define ARCVAE_PERSIST_BF16 2     /* arcvae_enc_lstm_forward_persistent flags bit 1 / arcvae_enc_lstm_backward_persistent_rs flags
                                   * bit 1: throughput mode for the persistent sweeps -- the 4x4 MFMA blocks (H 256, B <= 64
                                   * forward, B <= 128 BPTT) on v_mfma_f32_4x4x4_16b_bf16, weights and h / dG rounded to bf16
                                   * on their way into the instruction */
#define ARCVAE_RS_HALF 16         /* arcvae_enc_lstm_backward_persistent_rs flags bit 4: the half-batch form (129 <= B <= 256 where
                                   * arcvae_enc_lstm_bwd_rs_halves says so): this call sweeps rows 32 x + 16 half + [0, 16) of XCD x
                                   * only -- half = 0, or 1 with ARCVAE_RS_HALF1 -- and a chunk of the BPTT is TWO calls, one per
                                   * half, on the same stream with the same sync_ws / part_ws (a 16-row tick costs 4.0 us, the 32-row
                                   * block's 9.7) */
#define ARCVAE_RS_HALF1 32        /* ... flags bit 5: the second half */
#define ARCVAE_DEC_SPLIT3 512     /* arcvae_dec_forward_dense `mode` bit 9 / arcvae_dec_backward_dense `flags` bit 9: the B*V-row
                                   * products with ARCVAE_GEMM_SPLIT3 (fp32-class accuracy, less matrix-pipe time beside a sweep) */
#define ARCVAE_DEC_NO_GPRE 1024   /* arcvae_dec_forward_dense `mode` bit 10: forward only (sampler, loss-only forward) -- `gpre` is not
                                   * written: a layer's GEMM and zero-state cell run as one kernel where the shape allows */
#define ARCVAE_DEC_PART_HEAD 2048 /* arcvae_dec_forward_dense `mode` / arcvae_dec_backward_dense `flags` bit 11: only the token table and
                                     layer 0 (forward: tableD, hact[0]; backward: from dh_0 in dh[0 .. B*V*H)) */
#define ARCVAE_DEC_PART_TAIL 4096 /* bit 12: only fc_out (forward: logits, lse, nxt from hact[L-1]; backward: dWout, dbout and
                                     dh_top = dlogits . Wout into dh[0 .. B*V*H)); the caller runs layers 1 .. L-1 in between:
                                     arcvae_dense_stack_forward / _backward */
#define ARCVAE_DEC_BF16 256       /* arcvae_dec_forward_dense `mode` bit 8 / arcvae_dec_backward_dense `flags` bit 8: the B*V-row
                                   * products with ARCVAE_GEMM_BF16 */

/* A hipStream_t.  Callers without the HIP headers pass it as void*; the library's own translation units include this header
 * too (csrc/common.h defines ARCVAE_HIP_BUILD behind <hip/hip_runtime.h>), so a declaration here that drifts from its
 * definition in csrc/ is a compile error ("conflicting declaration of C function"), not a silent ABI mismatch. */
#ifdef ARCVAE_HIP_BUILD
typedef hipStream_t arcvae_stream_t;
#else
typedef void* arcvae_stream_t;
#endif

/* ABI version / build probe: returns 1000*major + minor; *arch_gfx950 = 1 when the code object
 * was built for gfx950. */
int arcvae_abi_version(int* arch_gfx950);

/* ---- generic contraction (MLX addmm / matmul, M2: y = x W^T + b) -------------------------
 * C[M,N] (+)= op(A) op(B) (+ bias[N]); transA=0: A [M,K], transA=1: A stored [K,M];
 * transB=0: B [K,N], transB=1: B stored [N,K].  Replaces every nn.Linear / matmul on the path,
 * e.g. models/encoder.py:109,115,117,118 and models/decoder.py:175. */
int arcvae_gemm_f32(int transA, int transB, int M, int N, int K, const float* A, int lda,
                    const float* B, int ldb, float* C, int ldc, const float* bias, int flags,
                    arcvae_stream_t stream);

/* ---- encoder LSTM stack -------------------------------------------------------------------
 * models/encoder.py:93-101: embedding lookup + L stacked nn.LSTM over the full padded sequence
 * (MLX nn.LSTM semantics M1: gates i,f,g,o; t=0 has no recurrent term and c_0 = i*g).
 * x_tb [T,B] int32 tokens (time-major; arcvae_transpose_tokens makes it from [B,T]);
 * table0 [V,4H] = embedding . Wx_0^T + bias_0 (one arcvae_gemm_f32 call);
 * outputs hseq,cseq [L,T,B,H], gseq [L,T,B,4H] (post-activation gates, saved for BPTT);
 * workspaces: hseq_t [L, slots, B*H*q] -- the k-chunk-major operand copy of h_t in ring slot t % slots -- and wt [(2L-1), 4H*H*q],
 * the k-chunk-major weight copies, where q = 3/2 in the three-piece form (ARCVAE_LSTM_SPLIT3 where the shape runs on the tile
 * kernels: three bf16 planes per value) and 1 otherwise, and slots = arcvae_enc_lstm_operand_slots(B, T, H, L, flags): min(T, 16),
 * or T where the weight gradients read the operand planes.  The library decides q and slots from (B, H, L, flags) and the
 * ARCVAE_* kernel-family knobs at EVERY call, so the caller states what it allocated: ws_floats[4] = capacities in floats of
 * {hseq_t, dG_t, wt, wT} (HOST array; entries of buffers a call does not use are ignored).  A call whose kernel family needs more
 * than that returns ARCVAE_ERR_ARG before launching anything -- never a write past the buffer.  arcvae_enc_lstm_ws_floats
 * returns the sizes needed under the current knobs. */
int arcvae_enc_lstm_ws_floats(int B, int T, int H, int L, int flags, long* floats /* out [4]: hseq_t, dG_t, wt, wT */);
int arcvae_transpose_tokens(const int32_t* src_bt, int32_t* dst_tb, int B, int T, arcvae_stream_t stream);
int arcvae_enc_lstm_forward(const int32_t* x_tb, const float* table0, const float* const* Wx,
                            const float* const* Wh, const float* const* bias, float* hseq, float* hseq_t,
                            float* cseq, float* gseq, float* wt, float* wT_bwd /* optional */, int B, int T, int V,
                            int H, int L, int flags /* ARCVAE_LSTM_SPLIT3, ARCVAE_LSTM_BF16 or 0; the same value must go to the
                            backward */, const long* ws_floats /* [4] capacities: hseq_t, -, wt, wT_bwd */,
                            void* h_oct /* optional, throughput mode: [L,T*B/8,H,8] bf16 "octet-major" copy of hseq
                            (k = t*B + b in groups of 8 per row: the layout an MFMA fragment is loaded in) for
                            arcvae_enc_lstm_wgrad; written when the tiled bf16 kernels run and B % 16 == 0 */,
                            unsigned long long* trace /* optional diagnostic: {start,end} 100 MHz stamps
                            of launch s at trace[2s..2s+1], 2*(T+L-1) u64 */, arcvae_stream_t stream);
/* bit 0 / bit 1: the forward / backward sweep of this shape runs on the register-tiled step kernels, i.e. ARCVAE_LSTM_BF16
 * takes effect there and h_oct / dG_oct get written (pass them to arcvae_enc_lstm_wgrad only when both bits are set). */
int arcvae_enc_lstm_tiled(int B, int H, int L);
/* The same for sweeps called with `flags`: with ARCVAE_LSTM_SPLIT3 (the three-piece form, what the engine passes on the parity path)
 * the tile regime starts at smaller grids -- from ~768 rows per GPU at H 256 / L 2 instead of ~1100. */
int arcvae_enc_lstm_tiled_for(int B, int H, int L, int flags);
/* Time slots of the operand rings hseq_t [L,slots,..] / dG_t [L,slots,..] the sweeps use for this shape with these flags: T where
 * the weight gradients read the operand planes (both sweeps on the three-piece tile kernels, B % 32 == 0: pass the rings to
 * arcvae_enc_lstm_wgrad with parts bit 11), else min(T, 16).  The dc / dX rings always have min(T, 16) slots. */
int arcvae_enc_lstm_operand_slots(int B, int T, int H, int L, int flags);
/* Backward of the above (the part of mx.value_and_grad, trainer.py:292, that walks the encoder
 * LSTM graph).  dh_top [B, ld_dh_top]: gradient w.r.t. the top layer's h at t = T-1, the only
 * position read by models/encoder.py:106.  dG out [L,T,B,4H] (may alias gseq: in-place); dG_t ws [L,slots,B*4H*q] and wT ws
 * [(2L-1),H*4H*q] with slots and q as for the forward (capacities in ws_floats[1] and [3]); dcs, dxs ws [L,RS,B,H], rings over t
 * with RS = min(T,16) slots (ARCVAE_RING) whatever the form: a slab is consumed by the next launch only. */
int arcvae_enc_lstm_backward(const float* const* Wx, const float* const* Wh, const float* cseq,
                             const float* gseq, const float* dh_top, int ld_dh_top, float* dG, float* dG_t,
                             float* dcs, float* dxs, float* wT, int B, int T, int H, int L, int s_begin,
                             int s_end, int flags /* ARCVAE_LSTM_RETILE | ARCVAE_LSTM_SPLIT3 or ARCVAE_LSTM_BF16 */,
                             const long* ws_floats /* [4] capacities: -, dG_t, -, wT */,
                             void* dG_oct /* optional, throughput mode: [L,T*B/8,4H,8] bf16 octet-major copy of dG */,
                             unsigned* start_signal /* optional: += 1 when the first launch of
                             this call starts (all earlier work of the stream is complete) */,
                             unsigned long long* trace /* optional diagnostic: stamps of launch s at trace[2s..2s+1],
                             2*(T+2(L-1)) u64 */, arcvae_stream_t stream);
/* The same forward sweep as ONE persistent launch for the latency regime (H = 128, 256 or 384, L <= 4, B <= 256, weight
 * slices within LDS; arcvae_enc_lstm_persistent_ok says whether a shape qualifies): batch rows partitioned over the 8
 * XCDs, weights stationary in LDS, one flag-line barrier per XCD and tick.  No k-chunk-major h
 * copy is written.  sync_ws: 8192 u32 of scratch (forward: words [0, 272); the BPTT entry points: [512, 848); [500] = the
 * error word of both); sync_ws[500] != 0 afterwards = a block gave up waiting (sticky).
 * start_signal (optional): += 1 when the sweep starts.  The BPTT counterpart covers ticks [s_begin, s_end) of
 * arcvae_enc_lstm_backward's schedule per launch (L <= 2, ceil(B/8) * H/32 <= 64); a sweep uses it for all its
 * chunks or for none (no k-chunk-major dG copy is written).  chunk_index: 0 for the launch with s_begin == 0 (it
 * re-arms sync_ws), then 1, 2, .. (< 8) for the following chunk launches of the same sweep: every chunk launch draws
 * its block roles from its own counters.  trace (optional diagnostic): per-tick {start,end} stamps of one block at
 * trace[2s..2s+1] (forward: s < T+L-1; BPTT: the sweep's global tick index s < T+2(L-1)). */
int arcvae_enc_lstm_persistent_ok(int B, int T, int H, int L);
/* (the sweep reads the row-major Wx / Wh themselves: no k-chunk-major copy.  wT_bwd, optional: also write the BPTT
 * layouts for a launch-based arcvae_enc_lstm_backward(retile = 0) of the same step.  flags bit 0: sync_ws has been
 * re-armed by arcvae_enc_prologue; bit 1: ARCVAE_PERSIST_BF16.) */
int arcvae_enc_lstm_forward_persistent(const int32_t* x_tb, const float* table0, const float* const* Wx,
                                       const float* const* Wh, const float* const* bias, float* hseq, float* cseq,
                                       float* gseq, float* wT_bwd, long wT_bwd_floats /* capacity of wT_bwd in floats (entry [3] of
                                       arcvae_enc_lstm_ws_floats); ignored when wT_bwd is NULL */, float* comb /* optional [B,2H]: its first H columns
                                       receive h_{T-1} of the top layer, the heads' input (models/encoder.py:106) */,
                                       unsigned* sync_ws, unsigned* start_signal, int B, int T, int V, int H, int L,
                                       int flags, unsigned long long* trace, arcvae_stream_t stream);
/* The byte-moving launches in front of the persistent forward sweep as one: x_tb = x_bt^T (arcvae_transpose_tokens),
 * zero_f32[0..n_zero) = 0 (optional: the encoder's gradient buffer), sync_ws[0..n_sync) = 0 (optional: the sweep's
 * re-arm). */
/* cond .. stats (optional, all or none): also comb[:, H:2H] = condition_fc(cond) (models/encoder.py:109-112) and
 * stats[0..n_stats) = 0, for arcvae_enc_heads_forward(comb_ready = 1).  onehot_ws (optional, [T*B, roundup(V,4)]): the
 * one-hot token rows of arcvae_enc_lstm_wgrad (called with parts bit 5 then). */
int arcvae_enc_prologue(const int32_t* x_bt, int32_t* x_tb, float* zero_f32, long n_zero, float* zero2_f32 /* optional second
                        zero fill: the token-table workspaces of arcvae_enc_lstm_wgrad (parts bit 8 then) */, long n_zero2,
                        unsigned* sync_ws, int n_sync, int sync_keep /* word index left alone, or -1: the sweeps' sticky error
                        word 500 when n_sync covers it -- 848 re-arms the forward AND the BPTT sweep of the step */,
                        const float* cond, const float* Wc, const float* bc, float* comb, float* stats, int n_stats,
                        float* onehot_ws, int V, int B, int T, int H, int C, arcvae_stream_t stream);
int arcvae_enc_lstm_bwd_persistent_ok(int B, int T, int H, int L);
int arcvae_enc_lstm_backward_persistent(const float* cseq, const float* gseq, const float* dh_top, int ld_dh_top,
                                        float* dG, float* dcs, float* dxs, const float* wT, unsigned* sync_ws,
                                        unsigned* start_signal, int B, int T, int H, int L, int s_begin, int s_end,
                                        int chunk_index, unsigned long long* trace, arcvae_stream_t stream);
/* Reduce-scatter form of the persistent BPTT sweep (H = 256, L <= 2, B <= 256): a CU keeps the gate gradients of its own
 * 32 gate columns on chip, multiplies them with its 32 rows of the row-major Wh / Wx, and the partial sums are
 * reduce-scattered through the XCD's L2 (part_ws: RG*2*(2L-1)*8*32*32*64 floats, RG = 1 / 2 / 4 groups of 8 rows per
 * XCD for B <= 64 / 128 / 256).  Otherwise as arcvae_enc_lstm_backward_persistent. */
int arcvae_enc_lstm_bwd_rs_ok(int B, int T, int H, int L);
/* Floats of part_ws that sweep uses for this shape under the current knobs (0 where it does not run): pass the capacity the
 * caller allocated as part_ws_floats -- a call that would need more returns ARCVAE_ERR_ARG. */
long arcvae_enc_lstm_bwd_rs_part_floats(int B, int T, int H, int L);
/* 1 where that sweep runs as two half-batch sweeps per chunk (ARCVAE_RS_HALVES=1, 129 <= B <= 256): see ARCVAE_RS_HALF. */
int arcvae_enc_lstm_bwd_rs_halves(int B, int T, int H, int L);
/* 2 where the persistent sweeps run in their TWO-GROUP form (H = 256, L <= 2, 129 <= B <= 256: the 256-row shard of
 * BASELINE.json configs[3]), else 1.  Two groups: 512 blocks, two per CU; every XCD's 17..32 rows are two independent
 * recurrences of up to 16 rows with their own flag lines, and a CU's two blocks serve different groups, so that one group's
 * exchange latency sits under the other's matrix work.  Such a step uses sync_ws words [1024, 4352)
 * as well; a step re-arms 4864 words (arcvae_enc_prologue n_sync: the one-group words [0, 848), the two-group words and the
 * reduce-scatter sweep's "gathered" words [4352, 4864) of its single-buffered exchange); part_ws as for RG = 4. */
int arcvae_enc_lstm_persist_groups(int B, int H, int L);
int arcvae_enc_lstm_backward_persistent_rs(const float* const* Wx, const float* const* Wh, const float* cseq,
                                           const float* gseq, const float* dh_top, int ld_dh_top, float* dG, float* dcs,
                                           float* dxs, float* part_ws, long part_ws_floats, unsigned* sync_ws,
                                           unsigned* start_signal, int B, int T, int H, int L, int s_begin, int s_end, int chunk_index,
                                           int flags /* bit 0: sync_ws was re-armed ahead of the step (arcvae_enc_prologue with
                                           n_sync >= 848); bit 1: ARCVAE_PERSIST_BF16; bits 4, 5: ARCVAE_RS_HALF, ARCVAE_RS_HALF1 */,
                                           unsigned long long* trace,
                                           arcvae_stream_t stream);
/* The reduce-scatter sweep with the stack's weight gradients formed INSIDE the kernel: replaces
 * arcvae_enc_lstm_backward_persistent_rs + the per-layer GEMMs / bias sums / token segment-sum of arcvae_enc_lstm_wgrad
 * for the same ticks.  "+=" into dWh[l], dWx[l] (l >= 1), dbias[l] (l >= 1); the layer-0 input side arrives as
 * dtable_ws [V,4H] (zeroed by the chunk_index == 0 call) for arcvae_table_finalize.  hseq [L,T,B,H] and x_tb [T,B] as
 * written / read by the forward sweep; dWx, dWh, dbias: HOST arrays of device pointers.  Same shape rule as _rs. */
int arcvae_enc_lstm_backward_fused(const float* const* Wx, const float* const* Wh, const float* cseq, const float* gseq,
                                   const float* hseq, const int32_t* x_tb, const float* dh_top, int ld_dh_top,
                                   float* dG, float* dcs, float* dxs, float* part_ws, long part_ws_floats, unsigned* sync_ws,
                                   unsigned* start_signal, float* const* dWx, float* const* dWh, float* const* dbias,
                                   float* dtable_ws, int B, int T, int V, int H, int L, int s_begin, int s_end,
                                   int chunk_index, unsigned long long* trace, arcvae_stream_t stream);
/* (the sweep is T+2(L-1) dependent launches; [s_begin, s_end) selects a sub-range so the caller can interleave
 *  events: after launches [0, s_end) every layer has finished all t >= T - s_end + 2(L-1).)
 * Parameter gradients of the stack from dG over time range [t_lo, t_hi): embedding.weight,
 * lstm_layer_l.{Wx,Wh,bias}; `first` zeroes the token-table workspace, `last` folds it into the
 * embedding / layer-0 gradients.  dtable_ws [V,4H]; onehot_ws [T*B, roundup(V,4)] (one-hot token rows, written
 * when `first`: the token segment-sum runs as OneHot^T . dG_0 on the matrix cores).  `parts` selects disjoint pieces
 * that may run on different streams: bit 0 = per-layer GEMMs and bias sums (= bits 2 | 3), bit 1 = token-table path,
 * bit 2 = dWx_l (l >= 1) and bias sums only, bit 3 = dWh_l only; bit 4 = exact-f32 tile GEMMs instead of the split-bf16
 * kernel; bit 5 = onehot_ws was written by arcvae_enc_prologue; bit 6 = the split-bf16 kernel's 128-row tile (the range
 * runs behind the sweep, no sweep block is resident); bit 8 = dtable_ws was zeroed ahead of the call (arcvae_enc_prologue:
 * the zero-fill launch in front of a `first` range is skipped); bit 9 = the per-layer GEMMs of the split-bf16 path on its
 * LDS-staged "quiet" form (ARCVAE_GEMM_QUIET: fewer bytes and load instructions beside the bs-64 BPTT sweep; ignored with
 * bits 4, 6, 7, 10, 11); bit 10 = the per-layer GEMMs as three-piece tile GEMMs
 * (ARCVAE_GEMM_SPLIT3: fp32-class accuracy, for the MFMA-bound regime beside the tiled sweeps); bit 7 = throughput mode (one bf16 product per GEMM step instead of
 * the six of the split form: not a parity path); bit 11 = h_oct / dG_oct are the sweeps' three-plane operand rings hseq_t /
 * dG_t with ALL T time slots (arcvae_enc_lstm_operand_slots == T): the per-layer GEMMs read the planes directly (transposing
 * LDS reads, no f32 loads, no re-splitting; needs B % 32 == 0); bit 13 = `last` folds with arcvae_table_fold instead of
 * arcvae_table_finalize (the caller guarantees that no other launch updates dEmb, dWx[0] or dbias[0] meanwhile).  The token-table path is linear in dtable_ws, so a
 * time range may be given its own workspace and both `first` and `last` (zero, accumulate, fold) on any stream. */
int arcvae_enc_lstm_wgrad(const int32_t* x_tb, const float* emb, const float* Wx0, const float* hseq,
                          const float* dG, float* dtable_ws, float* onehot_ws, float* dEmb, float* const* dWx,
                          float* const* dWh, float* const* dbias, int B, int T, int V, int E, int H, int L,
                          int t_lo, int t_hi, int first, int last, int parts /* 1 layers | 2 token table */,
                          const void* h_oct, const void* dG_oct /* optional (both or none), with parts bit 7: the octet-major
                          bf16 copies the sweeps of this step wrote -- the per-layer GEMMs then read those */,
                          const long* ws_floats /* with parts bit 11 (h_oct / dG_oct are plane rings with all T slots: [L,T,B*H*3/2]
                          and [L,T,B*4H*3/2] floats): [0], [1] = their capacities in floats, checked -- ARCVAE_ERR_ARG when smaller;
                          may be NULL otherwise */, arcvae_stream_t stream);

/* ---- encoder heads + reparameterisation + latent loss ----------------------------------------
 * models/encoder.py:106-130 (condition_fc, fc_mu, fc_logvar_hidden, fc_logvar, tanh bounds),
 * models/encoder.py:147-153 (z = mu + eps*exp(logvar/2), eps injected), and the per-rank halves
 * of losses/kl.py:39-56 and losses/info.py:27-41.  stats [2Z+4] is zeroed and filled here.
 * comb_ready != 0: comb [B,2H] and the zeroed stats were written ahead of the call (arcvae_enc_prologue + the persistent
 * forward sweep): hT, cond, Wc, bc are not read. */
int arcvae_enc_heads_forward(const float* hT, const float* cond, const float* Wc, const float* bc,
                             const float* Wmu, const float* bmu, const float* Wlh, const float* blh,
                             const float* Wlv, const float* blv, const float* eps, float* comb, float* lh,
                             float* mu_raw, float* lv_raw, float* mu, float* logvar, float* z, float* stats,
                             int B, int H, int Z, int C, float free_bits, int comb_ready, arcvae_stream_t stream);
/* The whole SEAM between the two sweeps as ONE per-XCD launch (OPT-IN, ARCVAE_SEAM_FUSED=1: parity-green, measured slower than the
 * five launches it replaces -- csrc/latent.hip; latency regime: B <= 64, hidden_dim a multiple of 64 up to 256, latent_dim a
 * multiple of 32 up to 128; arcvae_enc_seam_ok says whether the engine is to use it): arcvae_enc_heads_forward (comb_ready form) + arcvae_latent_loss (with
 * gradients) + arcvae_enc_heads_backward (phase 1) -- models/encoder.py:106-153, complete_vae_loss.py:45-99 and the heads' backward
 * up to dcomb -- with the batch rows partitioned over the 8 XCDs as in the persistent sweeps, every weight slice requested into LDS
 * when the block starts, activations exchanged through the XCD's L2, and the batch statistics (Q11) as atomics plus one device-wide
 * arrival counter.  phases: 1 = forward part (leaves this process's partial `stats`), 2 = backward part from GLOBAL stats (a
 * data-parallel step all-reduces `stats` between the two launches), 3 = both in one launch.  comb [B,2H] complete; stats [2Z+4]
 * zeroed ahead of the forward part; sync_ws: the sweeps' scratch -- words [4864, 5696) are the seam's (flags bit 0: zeroed ahead of
 * the step by arcvae_enc_prologue with n_sync >= 5696); sync_ws[500] != 0 afterwards = a block gave up waiting (sticky). */
int arcvae_enc_seam_ok(int B, int H, int Z);
int arcvae_enc_seam(const float* comb, const float* Wmu, const float* bmu, const float* Wlh, const float* blh, const float* Wlv,
                    const float* blv, const float* eps, const float* hyper, float* lh, float* mu_raw, float* lv_raw, float* mu,
                    float* logvar, float* z, float* stats, float* scalars, float* dmu_raw, float* dlv_raw, float* dlh, float* dcomb,
                    unsigned* sync_ws, int B, int H, int Z, int T, float free_bits, int phases, int flags, arcvae_stream_t stream);
int arcvae_stats_set_recon(const float* rowloss, int B, float* stats, int Z, arcvae_stream_t stream);
/* complete_vae_loss.py:45-99 (+ losses/kl.py, losses/info.py reductions) from GLOBAL stats.
 * hyper [8] device: beta, lambda_collapse, lambda_mi, target_mi, free_bits; scalars [16] device out:
 * total, recon, kl, beta*kl, collapse, prop(0), lambda_prop*prop(0), mutual_info, mi_penalty.
 * dmu_raw/dlv_raw [B,Z] may be NULL (forward only). */
int arcvae_latent_loss(const float* stats, const float* hyper, const float* mu, const float* logvar,
                       float* scalars, float* dmu_raw, float* dlv_raw, int B, int Z, int T, float free_bits,
                       arcvae_stream_t stream);
/* recon = stats[2Z+3]/(B_global*T) and total, once the decoder's CE row sums are in stats (latent_loss may run
 * before that: the encoder's backward does not depend on the reconstruction term, Q2). */
/* guard_a / guard_b (optional, here and in arcvae_recon_finalize): device error words as in arcvae_adam_update; when
 * either is non-zero the nine loss scalars are set to NaN and scalars[15] = 1 (else scalars[15] = 0), so the host's
 * per-batch read of the loss (trainer.py:366) also carries the "stream order was lost" status. */
int arcvae_loss_finalize(const float* stats, float* scalars, int Z, int T, const unsigned* guard_a,
                         const unsigned* guard_b, arcvae_stream_t stream);
/* arcvae_stats_set_recon + arcvae_loss_finalize in one launch (single-process step: losses/recon.py:59-60 mean over
 * B*T and complete_vae_loss.py:76-82 total). */
int arcvae_recon_finalize(const float* rowloss, int B, float* stats, float* scalars, int Z, int T,
                          const unsigned* guard_a, const unsigned* guard_b, arcvae_stream_t stream);
int arcvae_enc_heads_backward(const float* cond, const float* Wmu, const float* Wlh, const float* Wlv,
                              const float* comb, const float* lh, const float* dmu_raw, const float* dlv_raw,
                              float* dlh, float* dcomb, float* dWc, float* dbc, float* dWmu, float* dbmu,
                              float* dWlh, float* dblh, float* dWlv, float* dblv, int B, int H, int Z, int C,
                              int phase /* 0 both, 1 dcomb chain, 2 parameter gradients */, arcvae_stream_t stream);

/* ---- stand-alone loss pieces (the reference's `losses` module called on arbitrary tensors) ----------
 * models/encoder.py:147-153; losses/kl.py:39-58 + losses/info.py:27-35 partial sums (krow [B] may
 * be NULL: per-sample free-bits KL); losses/recon.py:29-57 per-position CE; out[0] = scale*sum(x). */
int arcvae_reparameterize(const float* mu, const float* logvar, const float* eps, float* z, long n,
                          arcvae_stream_t stream);
int arcvae_latent_stats(const float* mu, const float* logvar, float* stats, float* krow, int B, int Z,
                        float free_bits, arcvae_stream_t stream);
int arcvae_ce_rows(const float* logits, const int32_t* targets, float* ce, long R, int V, arcvae_stream_t stream);
int arcvae_sum(const float* x, long n, float* out, float scale, arcvae_stream_t stream);

/* ---- decoder, vocabulary-dense ------------------------------------------------------------------
 * models/decoder.py:152-175: per step embed(token) ++ conditions -> L zero-state LSTM cells
 * (hidden=None, cell=None every call, Q1) -> fc_out.  logits_t depends only on (token_t, cond_b),
 * so all B*V (row, token) pairs are evaluated at once: logits [B*V,V], lse [B*V], nxt [B*V]
 * (mode 0: first argmax(logits), decoder.py:185; mode 1: first argmax(softmax(logits/temperature)),
 * decoder_sampling.py:110-117; | ARCVAE_DEC_BF16: throughput mode). */
int arcvae_dec_forward_dense(const float* emb, const float* const* Wx, const float* const* bias,
                             const float* Wout, const float* bout, const float* cond, float* tableD,
                             float* hact, float* gpre, float* logits, float* lse, int32_t* nxt, int B, int V,
                             int E, int C, int H, int L, int mode, float temperature, arcvae_stream_t stream);
/* models/decoder.py:146-185 teacher-forcing walk (coins[t] = np.random.rand() < ratio, Q5) fused
 * with losses/recon.py:29-60 row sums: fed [B,T], rowloss [B] = sum_t CE. */
int arcvae_dec_chain_ce(const int32_t* x, const uint8_t* coins, const int32_t* nxt, const float* lse,
                        const float* logits, int32_t* fed, float* rowloss, int B, int T, int V,
                        arcvae_stream_t stream);
/* d(recon)/d(dense logits); inv_count = 1/(B_global*T) (mean over ALL positions, Q3). */
int arcvae_dec_ce_backward(const int32_t* x, const int32_t* fed, const float* logits, const float* lse,
                           float* dlogits, int B, int T, int V, float inv_count, arcvae_stream_t stream);
/* out[b,t,:] = dense[b, fed[b,t], :]: the [B,T,V] logits of models/decoder.py:188. */
int arcvae_dec_gather_logits(const float* dense, const int32_t* fed, float* out, int B, int T, int V,
                             arcvae_stream_t stream);
/* models/decoder_sampling.py:85-123 greedy walk: tokens [B,max_len], first_end [B]. */
int arcvae_dec_sample_chain(const int32_t* nxt, int32_t* tokens, int32_t* first_end, int B, int V,
                            int max_len, int end_token, arcvae_stream_t stream);
/* EXTENSION (not in the reference, whose sampler is greedy: "for now, use argmax", models/decoder_sampling.py:115-116): true
 * categorical sampling, tokens[b,t] ~ Categorical(softmax(dense_logits[b, cur, :] / temperature)) walked from the start token,
 * uniform numbers from a counter-based generator keyed by (seed, row, step): the same seed and batch give the same molecules.  dense_logits [B*V, V] as written by arcvae_dec_forward_dense (mode 0); vocab_size <= 256; first_end as above. */
int arcvae_dec_sample_chain_categorical(const float* dense_logits, int32_t* tokens, int32_t* first_end, int B, int V, int max_len,
                                        int end_token, float temperature, unsigned long long seed, arcvae_stream_t stream);
/* ---- dense-table decoders: common contract ------------------------------------------------------------------------------
 * The entry points from here to arcvae_dec_swor decode, sample or score over the table arcvae_dec_forward_dense (mode 0) wrote.
 * All are EXTENSIONS with no reference counterpart (the reference decodes greedily); each comment below states what it adds.
 * Table  dense_logits [B*V, V] fp32: row b*V + c holds batch row b's logits after token c.  The decoder is stateless per step:
 *   given its conditions a batch row's generator is a first-order Markov chain over the V tokens, and rows b*V .. b*V+V-1 are
 *   its transition matrix.  lse [B*V] comes from arcvae_dec_row_lse at the same temperature.
 * Step term  lp(c, v) = fl(fl(x[b*V+c, v] * inv_temp) - lse[b*V+c]), inv_temp = fl(1.0f / temperature); a score accumulates as
 *   s <- fl(s + lp) from s = 0, one add per step in step order.  One IEEE fp32 operation at a time, no contraction: the score an
 *   entry point returns for a sequence is bit for bit what arcvae_dec_sequence_logprob returns for its tokens.  (The top-k / top-p
 *   sampler reads no lse: its scaled logit is the inner fl(x * inv_temp).)
 * Start token  0: step 0 reads row b*V.
 * Limits  B, max_len >= 1; 1 <= V <= 256 (a token fits in a byte); 1 <= K <= 32 where there is a K; 0 <= pad_token <= 255 and
 *   0 <= min_len <= max_len where there is one; temperature > 0; ws_bytes at least the entry point's *_ws_bytes query (caller-owned
 *   device scratch); no NULL pointer but those marked.  Anything else (a NaN included) is ARCVAE_ERR_ARG before any launch.
 *   Two limits differ, on purpose or by history: arcvae_dec_viterbi* / _chain_marginals / _chain_expect / _kbest* index by
 *   end_token and want 0 <= end_token < V and a FINITE temperature (arcvae_dec_row_costs: finite temperatures); the others only compare end_token (any value; one outside [0, V) never matches)
 *   and take temperature = +inf (inv_temp = 0: every row uniform).
 * Tie order  where candidates are ordered through an integer key, the key is the order-preserving image of the fp32 value, then
 *   the complement of the index: value descending, index ascending.  -0 == +0 but their images differ: top-k / top-p and
 *   arcvae_dec_swor fold -0 into +0 first, so the index decides; arcvae_dec_kbest* does not fold.
 * Seed  a DEVICE pointer to one 64-bit word, read by the kernel: a captured launch serves every seed.  Batch row b's generator key is
 *   mix64(seed ^ (b << 32)), mix64 the splitmix64 finaliser (x += 0x9e3779b97f4a7c15; x = (x ^ x >> 30) * 0xbf58476d1ce4e5b9;
 *   x = (x ^ x >> 27) * 0x94d049bb133111eb; x ^ x >> 31) in 64-bit wrapping arithmetic; a draw is the top 24 bits (>> 40) of a hash.
 * All keep no host state, allocate nothing, are asynchronous on `stream` and capture-safe, and use no atomics: repeated calls are
 * bitwise identical. */
/* Beam search and the table's own functions.
 * arcvae_dec_row_lse: lse[r] = logsumexp(dense_logits[r, :] / temperature) of the R dense rows.
 * arcvae_dec_beam_search: per batch row, width K; a live hypothesis proposes every token (end_token excluded while t < min_len), a
 * finished one its pad_token continuation at the same score; the K best are kept under (score desc, parent slot asc, token asc).
 * Outputs tokens [B, K, max_len] (pad_token after the first end_token), scores [B, K] descending, lengths [B, K] (first end_token
 * index + 1, max_len without one, 0 for an empty slot: score -inf, pad tokens).  ws: pre-pass lists and back-pointers.
 * arcvae_dec_sequence_logprob: out[b] = sum_{t<=e} lp(fed_t, x[b,t]) in order, fed_0 = 0, fed_t = x[b,t-1], e = the first t with
 * x[b,t] == end_token (T-1 without one); tokens outside [0, V) are clamped. */
int arcvae_dec_row_lse(const float* dense_logits, float* lse, long R, int V, float temperature, arcvae_stream_t stream);
int arcvae_dec_beam_ws_bytes(int B, int K, int max_len, long* bytes);
int arcvae_dec_beam_search(const float* dense_logits, const float* lse, int32_t* tokens, float* scores, int32_t* lengths, void* ws,
                           long ws_bytes, int B, int V, int K, int max_len, int min_len, int end_token, int pad_token,
                           float temperature, arcvae_stream_t stream);
int arcvae_dec_sequence_logprob(const float* dense_logits, const float* lse, const int32_t* tokens, float* out, int B, int T, int V,
                                int end_token, float temperature, arcvae_stream_t stream);
/* Exact MAP decoding and exact chain marginals of the chain the table defines.  Both want 0 <= end_token < V and a finite
 * temperature (common contract); ws of arcvae_dec_viterbi: the back pointers, bytes [B, max_len, V].
 * arcvae_dec_viterbi, per batch row.  Admissible sequences x_0 .. x_{n-1}: either x_{n-1} = end_token with no earlier end_token and
 *   n-1 >= min_len, or n = max_len with no end_token at all.  Score: the left-to-right fp32 sum s <- fl(s + lp(fed_t, x_t)) from
 *   s = 0, fed_0 = 0, fed_t = x_{t-1} (what arcvae_dec_sequence_logprob returns for the tokens).  Recursion, for v != end_token:
 *   a_0[v] = fl(0 + lp(0, v)), a_t[v] = max over u != end_token of fl(a_{t-1}[u] + lp(u, v)), back pointer = the LOWEST u that
 *   attains the maximum; the end candidate e_t of a step t >= min_len is the same maximum into v = end_token (e_0 = fl(0 +
 *   lp(0, end_token))).  Result: the candidates e_{min_len}, ..., e_{max_len-1}, then a_{max_len-1}[v] for v != end_token in
 *   ascending v, scanned in that order; the first one is taken and a later one replaces it only when strictly greater -- on ties
 *   the earliest-ending sequence wins, then the lowest last token.  tokens [B, max_len] = the sequence, pad_token after its end;
 *   length [B] = n; score [B] = its score.
 *   Exactness: x -> fl(x + c) is monotone (non-decreasing) in x for IEEE round-to-nearest, so the best fp32 score of a prefix
 *   ending in v extends to the best fp32 score of every continuation: a_t[v] IS the maximum of the contract score over all
 *   end-free prefixes x_0 .. x_t = v, and the result IS the maximum over all admissible sequences -- exactly, not approximately,
 *   and never below any beam width's best hypothesis under the same min_len.  (Monotone, not strictly: two prefixes may round to
 *   one score; the tie rules above then say which sequence is returned.)
 *   A row holding a NaN or an infinite logit is outside the contract; it still writes tokens in [0, V) (and pad_token).  V = 1
 *   with min_len = max_len admits no sequence: score -inf, length max_len, tokens 0.
 * arcvae_dec_chain_marginals: with p(c, v) = expf(lp(c, v)), alive[b, 0, v] = p(0, v) and alive[b, t, v] = sum over u != end_token
 *   of alive[b, t-1, u] * p(u, v) = P(token at step t is v and no end_token before t), alive [B, max_len, V].  fp32 sums in the
 *   kernel's own, fixed order; no atomics: repeated calls are bitwise identical.  alive[b, t, end_token] = P(length = t+1) of what
 *   arcvae_dec_sample_chain_categorical draws; sum over v != end_token of alive[b, max_len-1, v] = P(no end within max_len). */
int arcvae_dec_viterbi_ws_bytes(int B, int V, int max_len, long* bytes);
int arcvae_dec_viterbi(const float* dense_logits, const float* lse, int32_t* tokens, float* score, int32_t* length, void* ws,
                       long ws_bytes, int B, int V, int max_len, int min_len, int end_token, int pad_token, float temperature,
                       arcvae_stream_t stream);
int arcvae_dec_chain_marginals(const float* dense_logits, const float* lse, float* alive, int B, int V, int max_len, int end_token,
                               float temperature, arcvae_stream_t stream);
/* Exact expectations over the chain's OUTCOMES: entropy, cross-entropy, expected token counts and length, the mass max_len cuts
 * off -- closed forms on the forward recursion of arcvae_dec_chain_marginals (same p, same alive, same limits: 0 <= end_token < V,
 * finite temperatures); nothing is sampled and alive is not written to memory.
 * An outcome of row b is a sequence up to and including its first end_token, of length n <= max_len, or max_len tokens without
 * one.  For a per-state cost r[b, u] the expected total over an outcome of sum_t r(fed_t), fed_0 = 0, fed_t = x_{t-1}, is
 *   total_r[b] = r[b, 0] + sum over v != end_token of r[b, v] * cont[b, v],  cont[b, v] = sum_{t=0}^{max_len-2} alive[b, t, v]
 *   (the start row always counts, also when end_token == 0; the last step's tokens are never fed back).
 * arcvae_dec_row_costs: the costs of the R = B*V table rows.  h[r] = -sum_v p(r, v) * lp(r, v), the row's entropy: by the chain
 *   rule total_h is the entropy of the outcome distribution, in nats.  With a second table q (logits_q, lse_q from
 *   arcvae_dec_row_lse at temperature_q; same R and V; other conditions, another temperature or other weights)
 *   c[r] = -sum_v p(r, v) * lq(r, v): total_c is the cross-entropy -E_P[log Q] and KL(P || Q) = fl(total_c - total_h), not clamped:
 *   rounding may leave it slightly negative.  q is logits_q, lse_q and c: all three NULL or all three given; temperature_q is
 *   checked either way.  p = expf(lp) is formed once and a term whose p is 0 is skipped (its logarithm may be -inf; 0 * inf is
 *   not relied on).  h and c accumulate in the same loop by the same operations and the same fixed butterfly, so a q that is the
 *   p table at the same lse and temperature gives c == h bit for bit, hence total_c == total_h and a KL of exactly 0.
 * arcvae_dec_chain_expect: n_cost (0 .. 4) per-state costs, cost [n_cost, B*V] -> totals [B, n_cost] (cost and totals NULL iff
 *   n_cost == 0; a state whose cont is 0 contributes 0 whatever its cost holds); visits [B, V] or NULL: visits[b, v] =
 *   sum_{t=0}^{max_len-1} alive[b, t, v], the expected number of times v is emitted -- column end_token is P(ended within max_len)
 *   and the sum over v is the expected length, an open outcome counting max_len; open_mass [B] or NULL: the sum over
 *   v != end_token of alive[b, max_len-1, v].  At least one output must be asked for; an output whose pointer is NULL is not
 *   touched.  fp32 sums in the kernel's own, fixed order: repeated calls are bitwise identical. */
int arcvae_dec_row_costs(const float* logits_p, const float* lse_p, float temperature_p, const float* logits_q, const float* lse_q,
                         float temperature_q, float* h, float* c, long R, int V, arcvae_stream_t stream);
int arcvae_dec_chain_expect(const float* dense_logits, const float* lse, const float* cost, int n_cost, float* totals, float* visits,
                            float* open_mass, int B, int V, int max_len, int end_token, float temperature, arcvae_stream_t stream);
/* Exact K-best decoding: the K most probable admissible sequences per batch row of the same chain, by a list-Viterbi recursion.
 * The admissible sequences and the limits are those of arcvae_dec_viterbi.
 * Lists: a_t[v] is a list of at most K scores, non-increasing; rank r has the back pointer (u, r').  a_0[v] = [fl(0 + lp(0, v))].
 *   For t >= 1 the candidates into column v are fl(a_{t-1}[u][r'] + lp(u, v)) for every u != end_token and every non-empty rank r',
 *   enumerated in (u ascending, r' ascending) order; a_t[v] is the first K of a STABLE sort of them by score descending, i.e. the
 *   order is (score desc, u asc, r' asc).  An empty entry is -inf and is never a candidate.  After step t column end_token is
 *   emptied: the end token never continues.
 * Result: the result candidates arrive in this order: for t = min_len .. max_len-1 the list into end_token at step t, by rank
 *   ascending; then, for v != end_token ascending, the list a_{max_len-1}[v], by rank ascending.  The result is the first K of a
 *   stable sort of that sequence by score descending: on ties the earlier-ending sequence comes first, then the lower last token,
 *   then the lower rank.
 * Outputs: scores [B, K] descending; tokens [B, K, max_len] = the sequence followed back through the (u, r') pointers, pad_token
 *   after its end; lengths [B, K] = n.  A slot with no candidate (fewer than K admissible sequences) holds score -inf, length 0
 *   and pad tokens only, like an empty beam slot.
 * Exactness: x -> fl(x + c) is monotone, so a prefix dropped at (t, v) has K kept prefixes whose every common continuation scores
 *   at least as high.  Hence scores[b, :] IS the multiset of the K largest contract scores over all admissible sequences; the K
 *   sequences are pairwise distinct; each score is what arcvae_dec_sequence_logprob returns for its tokens; rank j is never below
 *   rank j of any K-wide beam under the same min_len; and with K = 1 the outputs equal arcvae_dec_viterbi's.  Monotone is not
 *   strictly monotone: among sequences whose fp32 scores tie, the rules above decide which are returned; no simple global order on
 *   sequences is promised.
 * A row holding a NaN or an infinite logit is outside the contract; it still writes only tokens in [0, V) or pad_token.
 * ws: caller-owned device scratch for the back pointers, two bytes (u, r') per (step, token, rank) of a row IN FLIGHT: the kernel
 *   runs at most ARCVAE_KBEST_ROWS_IN_FLIGHT workgroups, each looping over rows b = its index, + the grid size, ... and reusing
 *   its slice, so arcvae_dec_kbest_ws_bytes = min(B, ARCVAE_KBEST_ROWS_IN_FLIGHT) * 2 * max_len * V * K whatever B is. */
#define ARCVAE_KBEST_ROWS_IN_FLIGHT 1024 /* 256 CUs x 4 workgroups of 256 threads: what the LDS of the V 80 workload admits per CU */
int arcvae_dec_kbest_ws_bytes(int B, int V, int K, int max_len, long* bytes);
int arcvae_dec_kbest(const float* dense_logits, const float* lse, int32_t* tokens /*[B,K,max_len]*/, float* scores /*[B,K]*/,
                     int32_t* lengths /*[B,K]*/, void* ws, long ws_bytes, int B, int V, int K, int max_len, int min_len,
                     int end_token, int pad_token, float temperature, arcvae_stream_t stream);
/* Length-normalised exact decoding and the best sequence of every length, on the same chain.  The raw score is the common
 * contract's s; the admissible sequences, min_len, pad_token and the limits are those of arcvae_dec_viterbi / arcvae_dec_kbest,
 * whose workspace queries serve.
 * len_div: a DEVICE array of max_len fp32 divisors, entry n-1 for the sequences of length n (the end token counts; a sequence
 *   without one has n = max_len); NULL = all ones.  Entries must be finite and > 0; the kernels cannot refuse a device array, so
 *   the caller checks (models/decoder_sampling.py does); a violating array is outside the contract, and the kernels still write
 *   only tokens in [0, V) or pad_token.  A candidate's KEY is fl(raw / d_n): one correctly rounded IEEE fp32 division, never a
 *   reciprocal and a product.
 * Exactness: for a fixed n, x -> fl(x / d_n) is non-decreasing, so the best key among the sequences of length n is the key of
 *   the best raw score of that length -- the e_t the Viterbi recursion forms at step t = n-1 -- and the K best keys of a length
 *   are the keys of its K best raw scores.  The optimum over all lengths is a maximum over the max_len per-length winners.
 * arcvae_dec_viterbi_norm.  Recursion and back pointers as arcvae_dec_viterbi.  Candidates, in this order: the end candidates of
 *   the steps t = min_len .. max_len-1 with key fl(e_t / d[t]); then ONE open candidate, the maximum raw a_{max_len-1}[v] over
 *   v != end_token, the lowest v on a tie, with key fl(. / d[max_len-1]).  The first candidate is taken; a later one replaces it
 *   only when its key is strictly greater: the earliest end wins a tie.  (The open candidate is chosen on raw scores so that
 *   K = 1 of the list form below is this.)  Outputs: tokens [B, max_len], length [B]; score [B] = the key; raw_score [B] =
 *   bitwise what arcvae_dec_sequence_logprob returns for the tokens; by_length [B, max_len] (NULL allowed) = the raw e_t of EVERY
 *   step t, whatever min_len is: the best score of any sequence whose first end_token is at position t (length t+1), -inf
 *   where there is none; open_score [B] (NULL allowed) = the open candidate's raw score, -inf for V = 1.  With len_div all ones
 *   or NULL, tokens, length and score are bitwise arcvae_dec_viterbi's.
 * arcvae_dec_viterbi_trace.  Reads the back pointers an arcvae_dec_viterbi / _norm call with the same B, V, max_len left in `ws`
 *   (same ws_bytes check) and lengths [B] (device).  tokens [B, max_len] = the sequence that ends with end_token at position
 *   n_b - 1, followed back through the pointers, then pad_token; its raw score is by_length[b, n_b - 1].  n_b is CLAMPED into
 *   [0, max_len]; n_b = 0 writes pad tokens only.  One forward call serves any number of traces.
 * arcvae_dec_kbest_norm.  The lists a_t[v] and their back pointers as arcvae_dec_kbest, on raw scores.  Arriving lists, in this
 *   order: for t = min_len .. max_len-1 the list into end_token at step t, by rank; then the final list: the first K of the
 *   stable sort by raw score descending of a_{max_len-1}[v], v != end_token ascending, by rank.  An entry's key is
 *   fl(raw / d_n); keys within a list stay non-increasing.  Each list is merged stably into the running K-entry result BY KEY,
 *   the result's entries first on ties.  Outputs: scores [B, K] = the keys, descending; raw_scores [B, K]; tokens, lengths and
 *   empty slots (by raw score -inf: key and raw -inf, length 0, pad tokens) as arcvae_dec_kbest.
 *   Properties: scores[b, :] IS the multiset of the K largest keys over all admissible sequences (per length by the
 *   monotonicity above, across lengths by the merge); the K sequences are pairwise distinct; each raw_scores entry is what
 *   arcvae_dec_sequence_logprob returns for its tokens, bit for bit; K = 1 equals arcvae_dec_viterbi_norm; all-ones (or NULL)
 *   divisors equal arcvae_dec_kbest bitwise. */
int arcvae_dec_viterbi_norm(const float* dense_logits, const float* lse, const float* len_div /*[max_len] or NULL*/,
                            int32_t* tokens, float* score, float* raw_score, int32_t* length, float* by_length /*or NULL*/,
                            float* open_score /*or NULL*/, void* ws, long ws_bytes, int B, int V, int max_len, int min_len,
                            int end_token, int pad_token, float temperature, arcvae_stream_t stream);
int arcvae_dec_viterbi_trace(const void* ws, long ws_bytes, const int32_t* lengths /*[B]*/, int32_t* tokens /*[B,max_len]*/, int B,
                             int V, int max_len, int end_token, int pad_token, arcvae_stream_t stream);
int arcvae_dec_kbest_norm(const float* dense_logits, const float* lse, const float* len_div /*[max_len] or NULL*/,
                          int32_t* tokens /*[B,K,max_len]*/, float* scores /*[B,K]*/, float* raw_scores /*[B,K]*/,
                          int32_t* lengths /*[B,K]*/, void* ws, long ws_bytes, int B, int V, int K, int max_len, int min_len,
                          int end_token, int pad_token, float temperature, arcvae_stream_t stream);
/* Top-k / nucleus (top-p) truncated sampling.  Beyond the common limits: top_k >= 0 (0 = all V), 0 < top_p <= 1.
 * Scaled logits s_j = fl(x_j * inv_temp).  Order: token j precedes token i iff s_j > s_i, or s_j == s_i and j < i.
 * Top-k set K = the first min(top_k, V) tokens of that order.  Masses e_j = expf(s_j - max s), C_i = the fp32 inclusive prefix sum
 * of e over K in that order (summation order the kernel's), M_K = C_{|K|-1}.  Nucleus set P: position i of K is kept iff
 * fl(C_i - e_i) < fl(top_p * M_K) (the mass strictly before it is below the threshold); top_p = 1 keeps every position of K with
 * e_i > 0; position 0 is always kept; n = |P| = the first position that fails (|K| if none), so K and P are prefixes of the order.
 * arcvae_dec_topkp_rows: the truncated distribution of R table rows (rows[i] = a table-row id, clamped into [0, table_rows); rows
 *   NULL = rows 0 .. R-1, R <= table_rows): count[i] = n, tokens[i, 0..V) = the row's whole order, cum[i, p] = C_p for p < |K|,
 *   0 beyond.  It is the inspection point of the walk: both run the same device code and agree bit for bit.
 * arcvae_dec_sample_chain_topkp: per batch row b; step t at token c reads row b*V + c, u24 = mix64(row key + t) >> 40 (the
 *   generator of arcvae_dec_sample_chain_categorical), theta = fl(fl(u24 * 2^-24) * C_{n-1}), picks the first position i < n with
 *   C_i > theta (n-1 if none) and writes tokens[b, t] = its token; first_end as arcvae_dec_sample_chain (tokens after EOS are still
 *   generated).  ws: a pre-pass stores every table row's truncated distribution there; the walk reads it.  Rows holding a NaN or
 *   inf logit are outside the contract; they still write tokens in [0, V). */
int arcvae_dec_topkp_rows(const float* dense_logits, long table_rows, const int32_t* rows, long R, int V, float temperature,
                          int top_k, float top_p, int32_t* count, int32_t* tokens, float* cum, arcvae_stream_t stream);
int arcvae_dec_topkp_ws_bytes(int B, int V, int top_k, long* bytes);
int arcvae_dec_sample_chain_topkp(const float* dense_logits, int32_t* tokens, int32_t* first_end, void* ws, long ws_bytes, int B,
                                  int V, int max_len, int end_token, float temperature, int top_k, float top_p,
                                  const unsigned long long* seed, arcvae_stream_t stream);
/* Min-p, locally typical and minimum-length truncated sampling: further rules that write the lists the top-k / top-p walk reads.
 * Beyond the top-k / top-p limits: 0 <= min_p < 1 (0 = off); 0 < typical_p <= 1 (1 = off); typical_p < 1 requires top_p == 1 and
 * min_p == 0; 0 <= min_len <= max_len; min_len > 0 requires 0 <= end_token < V and V >= 2; ban_token is -1 (none) or in [0, V),
 * and a ban_token >= 0 requires V >= 2.
 * s, the order, K, e_i = expf(fl(s_i - s_0)), C and M_K as above, with one change: a banned token sorts behind every real token
 *   (the value part of its key is 0, like the padding beyond V; its index part is kept) and |K| = min(top_k or V, V - 1).
 * The s-descending family (typical_p == 1): the nucleus rule as above gives n_p; min-p keeps position i >= 1 of K iff
 *   e_i >= min_p (e_0 = 1 is the image of the row's largest probability, so e_i = p_i / p_max: renormalisation does not enter),
 *   n_m = the first position that fails (|K| if none); n = min(n_p, n_m).  With min_p = 0 and no banned token the rows and the
 *   walk are arcvae_dec_topkp_rows' / arcvae_dec_sample_chain_topkp's, bit for bit.
 * The typical family (typical_p < 1; Meister et al. 2022), over the same K in the same s-order: a_i = fl(s_i - s_0),
 *   l_i = fl(a_i - logf(M_K)) -- the log of the renormalised probability, from s and not from e, so finite where e_i underflows;
 *   H = fl(-(sum over K of fl(e_i * l_i)) / M_K), the fp32 sum in the kernel's own, fixed order; d_i = |fl(l_i + H)|.  Typical
 *   order: position i precedes i' iff d_i < d_i', or d_i == d_i' and i < i' (ties to the higher s, then the lower token).  e'_q, C'_q =
 *   the masses in that order and their fp32 inclusive prefix sums, M' = C'_{|K|-1}; position q is kept iff q == 0 or
 *   fl(C'_q - e'_q) < fl(typical_p * M'); n = the first position that fails (|K| if none).  A prefix rule, as the nucleus:
 *   the warper of HuggingFace transformers keeps the tokens that tie at the cut instead.
 * arcvae_dec_trunc_rows: as arcvae_dec_topkp_rows.  Typical family: tokens[i, :] = the typical order over K, then the rest of the
 *   s-order (a banned token last); cum = C'; dev [R, V] (NULL allowed): dev[i, q] = d of position q < |K|, 0 beyond; ent [R] (NULL
 *   allowed) = H.  The other family writes dev and ent as 0 where asked for.
 * arcvae_dec_sample_chain_trunc: the walk of arcvae_dec_sample_chain_topkp (same generator, theta and pick rule), where a step
 *   t < min_len reads the lists built with ban_token = end_token and a step t >= min_len the plain ones: no end token appears
 *   before position min_len.  This is the LOCAL mask of the usual minimum-length processor, not conditioning on a length >=
 *   min_len: it changes the measure that is sampled (a prefix keeps the probability it had, the end token's mass is shared out
 *   among the other tokens of its step).  ws: 1 + (min_len > 0) list sets of the top-k / top-p size. */
int arcvae_dec_trunc_rows(const float* dense_logits, long table_rows, const int32_t* rows, long R, int V, float temperature,
                          int top_k, float top_p, float min_p, float typical_p, int ban_token, int32_t* count, int32_t* tokens,
                          float* cum, float* dev, float* ent, arcvae_stream_t stream);
int arcvae_dec_trunc_ws_bytes(int B, int V, int top_k, int min_len, long* bytes);
int arcvae_dec_sample_chain_trunc(const float* dense_logits, int32_t* tokens, int32_t* first_end, void* ws, long ws_bytes, int B,
                                  int V, int max_len, int min_len, int end_token, float temperature, int top_k, float top_p,
                                  float min_p, float typical_p, const unsigned long long* seed, arcvae_stream_t stream);
/* N independent draws per batch row from ONE dense table: the i.i.d. sampler behind "N molecules for this condition row".  The
 * caller passes each distinct condition row once; the table and the lists are built once per row, whatever N is.
 * Lists: the pre-pass is that of arcvae_dec_sample_chain_trunc, unchanged: it truncates the B*V table rows into one list set, or
 *   two with min_len > 0, in the same workspace layout (arcvae_dec_sample_draws_ws_bytes = arcvae_dec_trunc_ws_bytes).  A list
 *   set holds per table row the count n, the tokens as bytes and the fp32 cumulative masses C.  With every rule off (top_k = 0,
 *   top_p = 1, min_p = 0, typical_p = 1) the lists hold the whole row: the categorical sampler in list arithmetic, bit-equal to
 *   top_p = 1.0 of arcvae_dec_sample_chain_topkp and NOT to arcvae_dec_sample_chain_categorical, whose arithmetic differs.
 * Draw keys, in 64-bit wrapping arithmetic: key(b, 0) = the row key of the common contract, mix64(seed ^ (b << 32));
 *   key(b, d) = mix64(key(b, 0) ^ (0xD1B54A32D192ED03 * d)) for d >= 1.  A pure function of (seed, b, d): never of N, of the
 *   launch shape or of which workgroup or lane runs the draw.
 * Step t of a draw at token c (the start token 0 at t = 0) reads table row b*V + c, in the banned set while t < min_len:
 *   u24 = mix64(key + t) >> 40, theta = fl(fl(u24 * 2^-24) * C_{n-1}) with n = min(max(count, 1), S), S the lists' row length; the
 *   pick is the FIRST position i < n with C_i > theta, n - 1 if there is none; the next token is min(tok[pick], V - 1).  This is
 *   the rule of arcvae_dec_sample_chain_topkp / _trunc, operation for operation.  (C need not be non-decreasing in fp32: the
 *   scan's association order can step it down by an ulp at a multiple of 4.  "First position" is the rule; a bisection is not.)
 * Outputs: tokens [B, N, max_len]; first_end [B, N] = the first step whose token is end_token, max_len without one.
 *   pad_token = -1: the walk continues past the end, as the walks above.  0 <= pad_token <= 255: the positions after the first
 *   end hold pad_token and the draw stops consuming steps; the tokens up to and including the first end and first_end are the
 *   same in both modes.
 * Consequences: draw 0 with pad_token = -1 IS arcvae_dec_sample_chain_trunc, bit for bit, for the same arguments and seed; the
 *   draws of a call with N are the first N draws of a call with any larger N.
 * Limits: the common contract's and those of arcvae_dec_sample_chain_trunc, plus N >= 1; B * N <= 2^31 - 1 (a draw's index is an
 *   int), B * (N + 255) <= 2^32 - 1 (the walk's launch: B * ceil(N / w) workgroups of w <= 256 threads) and B * N * max_len <= 2^60
 *   (output offsets are 64-bit); pad_token -1 or in [0, 255]; ws_bytes at least the query.
 *   Anything else is ARCVAE_ERR_ARG before any launch.
 * seed is a DEVICE word (one captured graph serves every seed).  Capture-safe, no atomics, no allocation; repeated calls are
 *   bitwise identical. */
int arcvae_dec_sample_draws_ws_bytes(int B, int V, int top_k, int min_len, long* bytes);
int arcvae_dec_sample_draws(const float* dense_logits, int32_t* tokens /*[B,N,max_len]*/, int32_t* first_end /*[B,N]*/, void* ws,
                            long ws_bytes, int B, int N, int V, int max_len, int min_len, int end_token,
                            int pad_token /* -1: none */, float temperature, int top_k, float top_p, float min_p, float typical_p,
                            const unsigned long long* seed, arcvae_stream_t stream);
/* Sampling WITHOUT replacement: K distinct sequences per batch row that are exactly a sample without replacement from the sequence
 * distribution arcvae_dec_sample_chain_categorical draws from (stochastic beam search: Kool, van Hoof and Welling, ICML 2019).
 * ws: the back pointers.  arcvae_dec_swor, per batch row b:
 *   Log-probability  of a hypothesis: phi, the common contract's score.
 *   Noise  a pure function of (seed, b, token prefix), never of beam slots or launch shape: h_root = the row key,
 *     h_child = mix64(h_parent + token + 1) in 64-bit wrapping arithmetic; n = h_child >> 40,
 *     u = (n + 0.5) * 2^-24, g = -log(-log(u)).  (n + 0.5 is not an fp32 number for n >= 2^23: there -log(u) is evaluated as
 *     -log1p(-(2^24 - n - 0.5) * 2^-24), so every u lies strictly inside (0, 1) and g is finite.)
 *   Root  phi = 0, perturbed value G = 0.
 *   Open parent (phi_S, G_S): proposes all V children c: phi_c = phi_S + lp(c), Gp_c = phi_c + g_c, Z = max_c Gp_c, and the
 *     conditioned value G_c = -log(exp(-G_S) - exp(-Z) + exp(-Gp_c)), evaluated stably as v = G_S - Gp_c + log1p(-exp(Gp_c - Z)),
 *     G_c = G_S - max(0, v) - log1p(exp(-|v|)); the child that attains Z gets exactly G_S, no child more.  (The kernel forms
 *     Gp_c - Z and G_S - Gp_c from lp_c + g_c and a carried r = G - phi, so neither cancels numbers of size |phi|.)
 *   Finished parent (its last token was end_token): absorbing; one continuation, pad_token, phi and G unchanged.
 *   Selection  the next beam is the K candidates that come first under (G desc, parent slot asc, token asc).
 *   Threshold  threshold[b] = the running maximum over the steps of the best rejected candidate's G = the (K+1)-th largest
 *     perturbed value over all complete sequences; -inf if nothing was ever rejected.
 *   End  when every slot is finished or empty, or at max_len; a sequence still open at max_len is a leaf (the leaves
 *     arcvae_dec_sample_chain_categorical draws from).
 *   Outputs  tokens [B, K, max_len] (pad_token after the first end_token), log_probs [B, K] = phi, perturbed [B, K] = G, descending,
 *     lengths [B, K] (first end_token index + 1, max_len without one), threshold [B].  A slot no sequence fills (K above the number
 *     of sequences): log_probs = perturbed = -inf, pad tokens, length 0.  The K sequences of a row are pairwise distinct; rank 0 is
 *     one exact sample and does not depend on K.  Starting the root at G = 0 draws the perturbed values GIVEN that the row's largest
 *     is 0 (rank 0's perturbed is 0): the sample and its order are exact.  For estimates the conditioning is taken out afterwards,
 *     exp(-G') = exp(-G) - 1 + E with E ~ Exp(1) (the caller's: E = -log(u) of mix64(h_root) is noise no sequence uses); then, with
 *     q_k = 1 - exp(-exp(phi_k - threshold')), sum_k exp(phi_k) / q_k * f(x_k) over the ranks above the threshold's is an unbiased
 *     estimate of E[f].
 *   Not offered: min_len, top-k / top-p, length penalties -- each changes the measure that is sampled. */
int arcvae_dec_swor_ws_bytes(int B, int K, int max_len, long* bytes);
int arcvae_dec_swor(const float* dense_logits, const float* lse, const unsigned long long* seed, int32_t* tokens /*[B,K,max_len]*/,
                    float* log_probs /*[B,K]*/, float* perturbed /*[B,K]*/, int32_t* lengths /*[B,K]*/, float* threshold /*[B]*/,
                    void* ws, long ws_bytes, int B, int V, int K, int max_len, int end_token, int pad_token, float temperature,
                    arcvae_stream_t stream);
/* Backward of arcvae_dec_forward_dense: embedding.weight, lstm_layer_l.{Wx,bias}, fc_out.{weight,bias}.
 * ws: dh [2,B*V,H], dG [B*V,4H], dtableD [V,4H], wcpart [V,4H,max(C,1)]. */
int arcvae_dec_backward_dense(const float* emb, const float* const* Wx, const float* const* bias,
                              const float* Wout, const float* cond, const float* tableD, const float* hact,
                              const float* gpre, const float* dlogits, float* dh, float* dG, float* dtableD,
                              float* wcpart, float* dEmb, float* const* dWx, float* const* dbias, float* dWout,
                              float* dbout, int B, int V, int E, int C, int H, int L, int flags /* ARCVAE_DEC_BF16 or 0 */,
                              arcvae_stream_t stream);

/* Layers 1 .. L-1 of the vocabulary-dense decoder -- zero-state cells over R = B*V rows (Q1: hidden = cell = None at every call), an
 * (L-1)-layer stack at T = 1 -- on the three-piece tile kernels of the encoder's sweeps (lstm_fwd_tile_kernel,
 * lstm_bwd_tile_ks3_kernel, wgrad_planes_kernel: three bf16 pieces per operand, six products, fp32-class accuracy), for the
 * MFMA-bound regime where the decoder's exact-f32 GEMMs would run beside the forward sweep.
 *   arcvae_dense_stack_ok: 1 where that path applies (R % 32 == 0, H % 64 == 0, L >= 2, grids that fill the chip);
 *   arcvae_dense_stack_ws_floats: *floats = size of `ws` in floats (operand planes of every layer's h, cell states, gate-gradient planes,
 *   weight planes);  forward: hact [L,R,H] with layer 0 given (arcvae_dec_forward_dense | ARCVAE_DEC_PART_HEAD), layers 1 ..
 *   written; gates [L-1,R,4H] POST-activation (the gpre workspace holds them in this mode);  backward: dh_top [R,H] in, dG [R,4H]
 *   scratch, dh0 [R,H] out (the input of arcvae_dec_backward_dense | ARCVAE_DEC_PART_HEAD), dWx[l] / dbias[l] += for l >= 1
 *   (HOST arrays [L], entry 0 unused), `ws` as the forward left it. */
int arcvae_dense_stack_ok(long R, int H, int L);
int arcvae_dense_stack_ws_floats(long R, int H, int L, long* floats /* out */);
int arcvae_dense_stack_forward(const float* const* Wx, const float* const* bias, float* hact, float* gates, float* ws,
                               long ws_floats /* capacity of ws in floats: >= arcvae_dense_stack_ws_floats, else ARCVAE_ERR_ARG */, long R,
                               int H, int L, int flags /* bit 0: forward only (sampler): nothing the backward needs is written;
                               ARCVAE_LSTM_BF16 (bit 1): throughput mode -- bf16 operand copies, one product (not a parity path) */,
                               arcvae_stream_t stream);
int arcvae_dense_stack_backward(const float* gates, const float* dh_top, float* dG, float* dh0, float* const* dWx,
                                float* const* dbias, float* ws, long ws_floats, long R, int H, int L, int flags /* ARCVAE_LSTM_BF16 or 0: as the
                                forward was called */, arcvae_stream_t stream);

/* ---- optimizer ------------------------------------------------------------------------------------
 * trainer.py:75-76,320,324: MLX optim.Adam, NO bias correction (Q7):
 * m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p = p - lr m / (sqrt(v) + eps), over a flat buffer.
 * guard_a / guard_b (optional): device error words (engine: the gates' ERR word and the persistent sweeps'
 * sync_ws[500]); when either is non-zero at execution time the update is skipped -- gradients formed after a lost
 * stream order must not reach the weights. */
int arcvae_adam_update(float* params, const float* grads, float* m, float* v, long n, double lr,
                       double beta1, double beta2, double eps, const unsigned* guard_a, const unsigned* guard_b,
                       arcvae_stream_t stream);

/* arcvae_recon_finalize + arcvae_adam_update as ONE launch (the exposed tail of the single-process step, trainer.py:320-366):
 * block 0 sums the CE rows into stats[2Z+3] and writes the recon / total scalars (NaN and scalars[15] = 1 when a guard word is set),
 * then the update as above (skipped on a guard). */
int arcvae_adam_update_finalize(float* params, const float* grads, float* m, float* v, long n, double lr, double beta1,
                                double beta2, double eps, const unsigned* guard_a, const unsigned* guard_b,
                                const float* rowloss, int B, float* stats, float* scalars, int Z, int T, arcvae_stream_t stream);

/* ---- property predictor head (an extension: the reference's branch cannot run) ------------------------
 * Extends complete_vae_loss.py:64-74 (`property_predictor(z)` + losses/prop.py:5-40 `property_prediction_loss`, with the
 * arity fixed) and trainer.py:75-76 (a third Adam, over the predictor).  Predictor: pred = fc2(tanh(fc1(z))),
 * W1 [Hp,Z], b1 [Hp], W2 [C,Hp], b2 [C]; prop_loss = mean over B*C of (pred - cond)^2 -> scalars[5], lambda_prop * prop_loss
 * -> scalars[6] (lambda_prop = hyper[5]).  1 <= Z <= 512, 1 <= C <= 8, 1 <= Hp <= 256, else ARCVAE_ERR_ARG.
 * ws: the per-row partials (B * (2 Hp + C + 1) floats, arcvae_prop_ws_floats); every call states its capacity in ws_floats
 * and an undersized one is ARCVAE_ERR_ARG. */
int arcvae_prop_ws_floats(int B, int Z, int C, int Hp, long* floats);
/* Forward only (PropertyPredictor.__call__, the loss forward): pred [B,C] (may be null when scalars is given) and, when
 * scalars is non-null, the two loss scalars (cond and hyper required).  Two launches when the loss is asked for. */
int arcvae_prop_forward(const float* z, const float* cond, const float* W1, const float* b1, const float* W2,
                        const float* b2, const float* hyper, float* pred, float* scalars, float* ws, long ws_floats,
                        int B, int Z, int C, int Hp, arcvae_stream_t stream);
/* Training, ONE launch on the step's chain behind arcvae_latent_loss (which wrote d_mu_raw / d_lv_raw): forward, per-row
 * dpred = lambda_prop * 2 (pred - cond) / (B C), and dz = d(lambda_prop * prop_loss)/dz folded INTO (+=) d_mu_raw / d_lv_raw
 * through z = mu + eps exp(logvar/2), mu = 2 tanh(mu_raw/2), logvar = tanh(lv_raw/2) - 1.  Leaves the partials in ws;
 * pred (optional) receives the predictions. */
int arcvae_prop_backward(const float* z, const float* cond, const float* eps, const float* mu_raw, const float* lv_raw,
                         const float* W1, const float* b1, const float* W2, const float* b2, const float* hyper,
                         float* d_mu_raw, float* d_lv_raw, float* pred, float* ws, long ws_floats, int B, int Z, int C,
                         int Hp, arcvae_stream_t stream);
/* The predictor's weight gradients and loss scalars from the partials of arcvae_prop_backward: sums over rows in an order
 * fixed by B alone (contiguous row slices, each in row order, added in slice order: bitwise repeatable).  The gradients are OVERWRITTEN ("="), unlike the rest of this ABI. */
int arcvae_prop_wgrad(const float* z, const float* ws, long ws_floats, const float* hyper, float* dW1, float* db1,
                      float* dW2, float* db2, float* scalars, int B, int Z, int C, int Hp, arcvae_stream_t stream);

/* ---- opt-in global-norm gradient clipping (an extension: the reference's _clip_gradients, trainer.py:490-522, sums nothing, Q6) --
 * The reference's intended rule: norm = sqrt(sum g^2) over every gradient the step applies; when norm > max_norm (a NaN norm
 * compares false) every gradient is multiplied by scale = max_norm / (norm + 1e-8), rounded once to fp32, before the Adam update
 * above.  Step 1, per store: arcvae_grad_sumsq writes P fp32 partial sums of g^2 (P and the element-to-partial assignment depend
 * on n alone: bitwise repeatable, aligned or not).  Step 2, per store: the clipped update -- every block sums ALL n_partials
 * partials of all stores (one buffer, one fixed order) and applies gs = g * scale with the un-bias-corrected Adam on gs; the
 * gradients are not written.  When `scalars` is non-null, block 0 writes the pre-clip norm to scalars[11] and the applied scale
 * (1 when not clipping) to scalars[12]; NaN in both when a guard word is set (the update is skipped, as above).
 * ARCVAE_ERR_ARG before any launch: null pointers, n <= 0, partials_cap < P, n_partials outside [1, 4096], max_norm <= 0 or
 * not finite. */
/* P = min(256, ceil(ceil(n / 4) / 256)) partials for n floats, n >= 1. */
int arcvae_grad_sumsq_partials(long n, long* count);
int arcvae_grad_sumsq(const float* grads, long n, float* partials, long partials_cap, arcvae_stream_t stream);
int arcvae_adam_update_clipped(float* params, const float* grads, float* m, float* v, long n, double lr, double beta1,
                               double beta2, double eps, const unsigned* guard_a, const unsigned* guard_b,
                               const float* partials, long n_partials, double max_norm, float* scalars, arcvae_stream_t stream);
/* arcvae_adam_update_finalize with the clip (scalars required: the loss scalars and scalars[11..12]). */
int arcvae_adam_update_finalize_clipped(float* params, const float* grads, float* m, float* v, long n, double lr,
                                        double beta1, double beta2, double eps, const unsigned* guard_a,
                                        const unsigned* guard_b, const float* rowloss, int B, float* stats, float* scalars,
                                        int Z, int T, const float* partials, long n_partials, double max_norm,
                                        arcvae_stream_t stream);

/* ---- learning-rate schedules: the rate as a device word (an extension: the reference trains at one rate, trainer.py:75-76) ----
 * The four update forms above with the learning rate READ FROM DEVICE MEMORY at execution time (lr_dev: one fp32 word), so that
 * a launch captured in a hipGraph serves every rate.  rowloss non-null selects the finalize part (arcvae_adam_update_finalize:
 * stats, scalars, B, Z, T required), partials non-null the clip part (arcvae_adam_update_clipped: scalars required); neither,
 * either or both.  Same expressions, order, grid and float4 / scalar-tail split as the by-value forms: with *lr_dev == (float)lr
 * the results are bitwise theirs.  When `scalars` is non-null, block 0 also writes scalars[13] = *lr_dev, the rate this launch
 * applied.  A word that is negative, infinite or NaN updates nothing (params, m, v untouched; scalars[13] shows the word; the
 * finalize and clip scalars are still written -- the same split as a guard word, but not poisoned).  A zero word is a valid
 * rate: m and v advance, params do not move.
 * ARCVAE_ERR_ARG before any launch: null params / grads / m / v / lr_dev, n <= 0; a finalize part with null stats or scalars
 * or non-positive B, Z or T; a clip part with null scalars, n_partials outside [1, 4096], max_norm <= 0 or not finite. */
int arcvae_adam_step(float* params, const float* grads, float* m, float* v, long n,
                     const float* lr_dev,            /* DEVICE, one fp32 word, read by the kernel */
                     double beta1, double beta2, double eps,
                     const unsigned* guard_a, const unsigned* guard_b,
                     const float* rowloss, int B, float* stats, float* scalars, int Z, int T,  /* finalize part: rowloss NULL = none */
                     const float* partials, long n_partials, double max_norm,                   /* clip part: partials NULL = none   */
                     arcvae_stream_t stream);

/* ---- exponential moving average of the weights (an extension: the reference evaluates and samples the last step's weights) ----
 * Each entry point is ONE launch over all of a model's flat stores (encoder, decoder, optional predictor): ema / params / a / b
 * and n are HOST arrays of `segments` device pointers and element counts.
 * update: for every element of every segment  e = e + fl(omd * fl(p - e)),  omd = (float)one_minus_decay rounded once, every
 * operation in fp32 in that order, no FMA; `params` is never written.  The caller passes 1 - decay, formed in double, not the
 * decay: 1 - 0.9999 formed in fp32 is 1.0001659e-4 -- the weight of a new value would be off by 1.7e-4 relative before the first
 * update.  When either guard word (optional device words, as in arcvae_adam_update) is non-zero at execution time nothing is
 * written: an update that Adam skipped does not pull the average either.
 * swap: exchanges the contents of a[i] and b[i] bit for bit; applied twice it is the identity.
 * Pointers need 4-byte alignment only: a segment whose two pointers are 16-byte aligned takes a float4 main loop and a scalar
 * tail, any other the scalar loop.  Both keep no host state, allocate nothing and are capture-safe.
 * ARCVAE_ERR_ARG before any launch: null arrays, segments outside [1, ARCVAE_EMA_MAX_SEGMENTS], an n[i] <= 0, a null pointer in a
 * used segment; for the update, one_minus_decay outside (0, 1] or not finite. */
#define ARCVAE_EMA_MAX_SEGMENTS 4
int arcvae_ema_update(float* const* ema, const float* const* params, const long* n, int segments, double one_minus_decay,
                      const unsigned* guard_a, const unsigned* guard_b, arcvae_stream_t stream);
int arcvae_ema_swap(float* const* a, float* const* b, const long* n, int segments, arcvae_stream_t stream);

/* ---- small helpers ---------------------------------------------------------------------------------- */
int arcvae_colsum_accum(const float* X, int rows, int cols, int ld, float* out, float scale,
                        arcvae_stream_t stream);
int arcvae_segsum_rows_accum(const float* X, const int32_t* seg, int rows, int nseg, int cols, float* out,
                             arcvae_stream_t stream);
int arcvae_transpose_batched(const float* const* src, float* const* dst, const int* rows, const int* cols,
                             int n, arcvae_stream_t stream);
/* Diagnostic / test entry point: `blocks` workgroups of `threads` threads (a multiple of 64) that hold `lds_bytes` of LDS each
 * and wait `spin_us` microseconds -- a stand-in for a communication kernel that occupies CU resources on another stream
 * beside the persistent sweeps (tests/test_occupancy_gpu.py).  Computes nothing. */
int arcvae_debug_occupy(int blocks, int threads, int lds_bytes, int spin_us, arcvae_stream_t stream);
int arcvae_scale_inplace(float* x, long n, float s, arcvae_stream_t stream);
int arcvae_zero(float* x, int rows, int cols, int ld, arcvae_stream_t stream);
/* Token-table gradient dT [V,4H] of an LSTM layer-0 input projection folded back in one launch (backward of
 * nn.Embedding + the x.Wx^T term of nn.LSTM, models/encoder.py:93,98 and models/decoder.py:154-166):
 * dEmb [V,E] += dT . Wx0[:, :E];  dWx0[:, :E] += dT^T . emb (row stride ldw);  db0 [4H] += colsum(dT). */
int arcvae_table_finalize(const float* dT, const float* Wx0, int ldw, const float* emb, float* dEmb, float* dWx0,
                          float* db0, int V, int E, int G, arcvae_stream_t stream);
/* The same three "+=" (same argument checks) on the exact-f32 MFMA forms with ONE owner per output element: no atomics,
 * a few KB of LDS, two runs bit-identical.  THE CALLER GUARANTEES that no other launch updates dEmb, dWx0[:, :E] or db0
 * while this one runs (arcvae_table_finalize's atomics allowed two folds at once; this one's plain "+=" does not).
 * dT2 (optional): a second table, the fold reads dT + dT2 (both 16-byte aligned).  [g_lo, g_hi) (both 0: none; else
 * multiples of 32 within [0, G]): columns of the table known to be zero -- they are not read (a gap in K for dEmb) and
 * rows [g_lo, g_hi) of dWx0 / db0 are not touched.  Columns E .. ldw-1 of dWx0 are never touched. */
int arcvae_table_fold(const float* dT, const float* dT2, const float* Wx0, int ldw, const float* emb, float* dEmb,
                      float* dWx0, float* db0, int V, int E, int G, int g_lo, int g_hi, arcvae_stream_t stream);
/* Device-side gates (no reference counterpart): cross-stream ordering by a one-wave polling kernel instead of an
 * event wait, because a hardware queue blocked on an event slows every dependent dispatch of the chain that is
 * running.  wait: returns once (int)(*flag - ((*steps) * stride + offset)) >= 0 (steps may be
 * NULL: target = offset); advance != 0: ++*steps afterwards; bounded spin of max_polls polls (~1 us each), on expiry
 * *err += 1.  set: *flag = value (add == 0) or *flag += value, ordered after the earlier work of the stream. */
int arcvae_gate_wait(const unsigned* flag, unsigned* steps, unsigned stride, unsigned offset, int advance,
                     unsigned max_polls, unsigned* err, arcvae_stream_t stream);
int arcvae_gate_set(unsigned* flag, unsigned value, int add, arcvae_stream_t stream);
int arcvae_tile_weights(const float* const* src, float* const* dst, const int* cols, const int* mode, int n, int H,
                        arcvae_stream_t stream);
/* n <= 8 small device-to-device copies in ONE launch (a step's inputs -- tokens, conditions, eps, coins -- were four copy
 * launches of ~4 us each in front of every step): dst_i[0..nbytes_i) = src_i[0..nbytes_i).  HOST arrays of pointers. */
int arcvae_copy_buffers(const void* const* src, void* const* dst, const long* nbytes, int n, arcvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ARCVAE_HIP_H */
