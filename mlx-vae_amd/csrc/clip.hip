// Opt-in global-norm gradient clipping (an extension, DESIGN.md section 10: the reference's `_clip_gradients` sums nothing, Q6).
//
//   norm = sqrt(sum of g^2) over every gradient the step applies (encoder, decoder, predictor);
//   norm > max_norm (NaN: false)  ->  every gradient is multiplied by scale = fp32(max_norm / (norm + 1e-8)) before Adam.
//
// Two kernels (DESIGN.md section 7 has where they run in the step):
//   grad_sumsq_kernel  one launch per store: P fp32 partial sums of g^2 (P = arcvae_grad_sumsq_partials(n)).  Thread t of
//                      block b owns the element quads q = b*256 + t + k*P*256 and adds their squares in element order, so the
//                      assignment and every partial depend on n alone -- float4 loads where the pointer allows, else four scalar
//                      loads of the same values in the same order: bitwise the same partials either way.
//   adam_clip_kernel   the un-bias-corrected Adam of misc.hip (adam_kernel), with a prologue: EVERY block sums all partials of
//                      all stores itself, in one fixed order (fp64), and derives the same norm and scale -- the launch boundary
//                      is the reduction's barrier: no float atomics, no last-block hand-off.  Block 0 writes the pre-clip norm
//                      to scalars[11] and the applied scale to scalars[12] (NaN, NaN on a tripped guard: nothing is applied).
// The gradient buffers themselves are never written: they keep the unclipped gradients.
#include "ops.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int CLIP_THREADS = 256;
constexpr long CLIP_MAX_PARTIALS = 256;     // per store (encoder 1.3 M floats: 256 blocks of 256 threads, five quads each)
constexpr long CLIP_MAX_TOTAL = 4096;       // partials one clipped update may reduce (all stores together)

long sumsq_partials(long n) {
    const long quads = (n + 3) / 4;
    const long p = (quads + CLIP_THREADS - 1) / CLIP_THREADS;
    return p < CLIP_MAX_PARTIALS ? p : CLIP_MAX_PARTIALS;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(CLIP_THREADS) void grad_sumsq_kernel(const float* __restrict__ g, long n, int vec,
                                                                  float* __restrict__ partials) {
#pragma clang fp contract(off)
    const long quads = (n + 3) >> 2;
    const long stride = (long)gridDim.x * CLIP_THREADS;
    float s = 0.f;
    for (long q = (long)blockIdx.x * CLIP_THREADS + threadIdx.x; q < quads; q += stride) {
        const long e = q * 4;
        float a, b, c, d;
        if (vec && e + 3 < n) {
            const float4 x = reinterpret_cast<const float4*>(g)[q];
            a = x.x; b = x.y; c = x.z; d = x.w;
        } else {
            a = g[e];
            b = e + 1 < n ? g[e + 1] : 0.f;
            c = e + 2 < n ? g[e + 2] : 0.f;
            d = e + 3 < n ? g[e + 3] : 0.f;
        }
        s += (a * a + b * b) + (c * c + d * d);
    }
    __shared__ float red[CLIP_THREADS / 64];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

struct ClipFinalize {            // as misc.hip's AdamFinalize: the single-process step's loss finalize in block 0
    const float* rowloss; float* stats; int B, Z, T;
};

// DEV: the device-rate form (arcvae_adam_step; misc.hip's adam_kernel has the contract): lr = *lr_dev, scalars[13] = lr.
template <bool DEV>
__global__ __launch_bounds__(CLIP_THREADS) void adam_clip_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                 float* __restrict__ m, float* __restrict__ v, long n4, long n,
                                                                 float lr_val, const float* lr_dev, float b1, float b2,
                                                                 float omb1, float omb2, float eps,
                                                                 const unsigned* guard_a, const unsigned* guard_b,
                                                                 const float* __restrict__ partials, int np, double max_norm,
                                                                 float* scalars, ClipFinalize fin) {
#pragma clang fp contract(off)
    const float lr = DEV ? *lr_dev : lr_val;
    const bool tripped = (guard_a && __hip_atomic_load(guard_a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) ||
                         (guard_b && __hip_atomic_load(guard_b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u);
    // the launch-boundary reduce: every block, all partials, one order
    __shared__ double dred[CLIP_THREADS / 64];
    double t = 0.0;
    for (int i = threadIdx.x; i < np; i += CLIP_THREADS) t += (double)partials[i];
    t = wave_sum_f64(t);
    if ((threadIdx.x & 63) == 0) dred[threadIdx.x >> 6] = t;
    __syncthreads();
    const float norm = (float)sqrt((dred[0] + dred[1]) + (dred[2] + dred[3]));
    const bool active = (double)norm > max_norm;                    // a NaN norm compares false: no scaling
    const float scale = active ? (float)(max_norm / ((double)norm + 1e-8)) : 1.0f;
    if (blockIdx.x == 0) {
        if (fin.rowloss) {
            float s = 0.f;
            for (int i = threadIdx.x; i < fin.B; i += CLIP_THREADS) s += fin.rowloss[i];
            __shared__ float red[CLIP_THREADS / 64];
            s = wave_sum(s);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
            __syncthreads();
            if (threadIdx.x == 0) {
                float* sc = scalars;
                const float ce = (red[0] + red[1]) + (red[2] + red[3]);
                fin.stats[2 * fin.Z + 3] = ce;
                const float recon = ce / (fin.stats[2 * fin.Z + 2] * (float)fin.T);
                sc[1] = recon;
                sc[0] = recon + sc[3] + sc[4] + sc[6] + sc[8];
                sc[15] = 0.0f;
                if (tripped) {
                    for (int i = 0; i < 9; ++i) sc[i] = __builtin_nanf("");
                    sc[15] = 1.0f;
                }
            }
        }
        if (scalars && threadIdx.x == 0) {
            scalars[11] = tripped ? __builtin_nanf("") : norm;
            scalars[12] = tripped ? __builtin_nanf("") : scale;
            if (DEV) scalars[13] = lr;
        }
    }
    if (tripped) return;
    if (DEV && !(lr >= 0.f && lr <= 3.402823466e+38f)) return;      // negative, infinite, NaN: nothing is updated
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 pp = reinterpret_cast<float4*>(p)[i];
        float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i];
        float4 vv = reinterpret_cast<float4*>(v)[i];
        if (active) {
            gg.x = gg.x * scale; gg.y = gg.y * scale; gg.z = gg.z * scale; gg.w = gg.w * scale;
        }
#define ADAM1(c)                                   \
        mm.c = b1 * mm.c + omb1 * gg.c;            \
        vv.c = b2 * vv.c + omb2 * (gg.c * gg.c);   \
        pp.c = pp.c - (lr * mm.c) / (sqrtf(vv.c) + eps);
        ADAM1(x) ADAM1(y) ADAM1(z) ADAM1(w)
#undef ADAM1
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
    }
    // scalar tail
    for (long i = n4 * 4 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float gi = active ? g[i] * scale : g[i];
        const float mi = b1 * m[i] + omb1 * gi;
        const float vi = b2 * v[i] + omb2 * (gi * gi);
        m[i] = mi;
        v[i] = vi;
        p[i] = p[i] - (lr * mi) / (sqrtf(vi) + eps);
    }
}

int launch_adam_clip(float* params, const float* grads, float* m, float* v, long n, double lr, const float* lr_dev,
                     double beta1, double beta2,
                     double eps, const unsigned* guard_a, const unsigned* guard_b, const float* partials, long n_partials,
                     double max_norm, float* scalars, ClipFinalize fin, hipStream_t stream) {
    const uintptr_t al = reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grads) |
                         reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v);
    const long n4 = (al & 15) ? 0 : n / 4;
    const float omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);   // as arcvae_adam_update
    const long work = n4 > 0 ? n4 : n;
    const int blocks = (int)std::min((long)2048, (work + 255) / 256);
    if (lr_dev)
        hipLaunchKernelGGL(adam_clip_kernel<true>, dim3(blocks), dim3(CLIP_THREADS), 0, stream, params, grads, m, v, n4, n, 0.f,
                           lr_dev, (float)beta1, (float)beta2, omb1, omb2, (float)eps, guard_a, guard_b, partials,
                           (int)n_partials, max_norm, scalars, fin);
    else
        hipLaunchKernelGGL(adam_clip_kernel<false>, dim3(blocks), dim3(CLIP_THREADS), 0, stream, params, grads, m, v, n4, n,
                           (float)lr, (const float*)nullptr, (float)beta1, (float)beta2, omb1, omb2, (float)eps, guard_a, guard_b,
                           partials, (int)n_partials, max_norm, scalars, fin);
    return arcvae_launch_status();
}

bool clip_args_ok(const float* partials, long n_partials, double max_norm) {
    return partials && n_partials >= 1 && n_partials <= CLIP_MAX_TOTAL && max_norm > 0.0 && std::isfinite(max_norm);
}

}  // namespace

extern "C" int arcvae_grad_sumsq_partials(long n, long* count) {
    if (n <= 0 || !count) return ARCVAE_ERR_ARG;
    *count = sumsq_partials(n);
    return ARCVAE_OK;
}

extern "C" int arcvae_grad_sumsq(const float* grads, long n, float* partials, long partials_cap, hipStream_t stream) {
    if (!grads || n <= 0 || !partials) return ARCVAE_ERR_ARG;
    const long P = sumsq_partials(n);
    if (partials_cap < P) return ARCVAE_ERR_ARG;
    const int vec = (reinterpret_cast<uintptr_t>(grads) & 15) ? 0 : 1;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)P), dim3(CLIP_THREADS), 0, stream, grads, n, vec, partials);
    return arcvae_launch_status();
}

extern "C" int arcvae_adam_update_clipped(float* params, const float* grads, float* m, float* v, long n, double lr,
                                          double beta1, double beta2, double eps, const unsigned* guard_a,
                                          const unsigned* guard_b, const float* partials, long n_partials, double max_norm,
                                          float* scalars, hipStream_t stream) {
    if (!params || !grads || !m || !v || n <= 0 || !clip_args_ok(partials, n_partials, max_norm)) return ARCVAE_ERR_ARG;
    ClipFinalize fin;
    fin.rowloss = nullptr; fin.stats = nullptr; fin.B = fin.Z = fin.T = 0;
    return launch_adam_clip(params, grads, m, v, n, lr, nullptr, beta1, beta2, eps, guard_a, guard_b, partials, n_partials, max_norm,
                            scalars, fin, stream);
}

extern "C" int arcvae_adam_update_finalize_clipped(float* params, const float* grads, float* m, float* v, long n, double lr,
                                                   double beta1, double beta2, double eps, const unsigned* guard_a,
                                                   const unsigned* guard_b, const float* rowloss, int B, float* stats,
                                                   float* scalars, int Z, int T, const float* partials, long n_partials,
                                                   double max_norm, hipStream_t stream) {
    if (!params || !grads || !m || !v || n <= 0 || !rowloss || !stats || !scalars || B <= 0 || Z <= 0 || T <= 0 ||
        !clip_args_ok(partials, n_partials, max_norm))
        return ARCVAE_ERR_ARG;
    ClipFinalize fin;
    fin.rowloss = rowloss; fin.stats = stats; fin.B = B; fin.Z = Z; fin.T = T;
    return launch_adam_clip(params, grads, m, v, n, lr, nullptr, beta1, beta2, eps, guard_a, guard_b, partials, n_partials, max_norm,
                            scalars, fin, stream);
}

// Every update form with the learning rate read from DEVICE memory (learning-rate schedules): one captured
// launch serves every rate.  rowloss non-null: the finalize part (arcvae_adam_update_finalize); partials non-null: the clip part
// (arcvae_adam_update_clipped); both: arcvae_adam_update_finalize_clipped.  With *lr_dev == (float)lr bitwise the by-value forms.
extern "C" int arcvae_adam_step(float* params, const float* grads, float* m, float* v, long n, const float* lr_dev,
                                double beta1, double beta2, double eps, const unsigned* guard_a, const unsigned* guard_b,
                                const float* rowloss, int B, float* stats, float* scalars, int Z, int T,
                                const float* partials, long n_partials, double max_norm, hipStream_t stream) {
    if (!params || !grads || !m || !v || !lr_dev || n <= 0) return ARCVAE_ERR_ARG;
    if (rowloss && (!stats || !scalars || B <= 0 || Z <= 0 || T <= 0)) return ARCVAE_ERR_ARG;
    if (partials && (!scalars || !clip_args_ok(partials, n_partials, max_norm))) return ARCVAE_ERR_ARG;
    if (!partials)
        return arcvae_adam_step_plain(params, grads, m, v, n, lr_dev, beta1, beta2, eps, guard_a, guard_b, rowloss, B, stats,
                                      scalars, Z, T, stream);
    ClipFinalize fin;
    fin.rowloss = rowloss; fin.stats = stats; fin.B = B; fin.Z = Z; fin.T = T;
    return launch_adam_clip(params, grads, m, v, n, 0.0, lr_dev, beta1, beta2, eps, guard_a, guard_b, partials, n_partials,
                            max_norm, scalars, fin, stream);
}
