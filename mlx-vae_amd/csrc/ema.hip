// Exponential moving average of the weights (an extension): the shadow update and the exact exchange of
// a model's flat parameter buffers with their shadows, each as ONE launch over all of the model's stores (encoder, decoder,
// optional predictor).  HBM-bound streaming kernels: the update reads 8 B and writes 4 B per parameter, the swap moves 8 B
// each way; 16-byte accesses where a segment's pointers allow them.  No LDS, no cross-lane work, no host state.
#include "ops.h"
#include <algorithm>
#include <cmath>

namespace {

// The segments of one launch, by value.  One grid covers the concatenated work: segment s owns blocks [end of s-1, end of s)
// (unused slots repeat the last bound, so no block ever selects them).  n4: float4 pieces of the main loop, 0 when one of
// the segment's pointers is not 16-byte aligned (then the scalar loop covers all n elements).
struct EmaSeg {
    float* a;
    float* b;      // the update only reads it (params)
    long n, n4;
    int end;
};
// (named members, not an array: a block picks its segment with compares on kernel arguments, never with a computed index
// into them -- that form went through scratch memory)
struct EmaSegs {
    EmaSeg s0, s1, s2, s3;
};
static_assert(ARCVAE_EMA_MAX_SEGMENTS == 4, "EmaSegs holds four segments");

// This block's segment and its place in it.
struct EmaPlace {
    float* a; float* b; long n, n4, first, stride;
};
__device__ __forceinline__ EmaPlace ema_place(const EmaSegs& sg) {
    const int bid = blockIdx.x;
    const bool p1 = bid >= sg.s0.end, p2 = bid >= sg.s1.end, p3 = bid >= sg.s2.end;
    EmaPlace pl;
    pl.a = p3 ? sg.s3.a : p2 ? sg.s2.a : p1 ? sg.s1.a : sg.s0.a;
    pl.b = p3 ? sg.s3.b : p2 ? sg.s2.b : p1 ? sg.s1.b : sg.s0.b;
    pl.n = p3 ? sg.s3.n : p2 ? sg.s2.n : p1 ? sg.s1.n : sg.s0.n;
    pl.n4 = p3 ? sg.s3.n4 : p2 ? sg.s2.n4 : p1 ? sg.s1.n4 : sg.s0.n4;
    const int s_beg = p3 ? sg.s2.end : p2 ? sg.s1.end : p1 ? sg.s0.end : 0;
    const int s_end = p3 ? sg.s3.end : p2 ? sg.s2.end : p1 ? sg.s1.end : sg.s0.end;
    pl.first = (long)(bid - s_beg) * blockDim.x + threadIdx.x;
    pl.stride = (long)(s_end - s_beg) * blockDim.x;
    return pl;
}

// e = e + fl(omd * fl(p - e)): three fp32 roundings in this order, no FMA.  Nothing is written when a guard word is set
// (the read of adam_kernel: an update that Adam skipped must not pull the average either).
__global__ __launch_bounds__(256) void ema_update_kernel(EmaSegs sg, float omd, const unsigned* guard_a,
                                                         const unsigned* guard_b) {
#pragma clang fp contract(off)
    const bool tripped = (guard_a && __hip_atomic_load(guard_a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) ||
                         (guard_b && __hip_atomic_load(guard_b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u);
    if (tripped) return;
    const EmaPlace pl = ema_place(sg);
    float* e = pl.a;
    const float* p = pl.b;
    for (long i = pl.first; i < pl.n4; i += pl.stride) {
        float4 ee = reinterpret_cast<float4*>(e)[i];
        const float4 pp = reinterpret_cast<const float4*>(p)[i];
#define EMA1(c) ee.c = ee.c + omd * (pp.c - ee.c);
        EMA1(x) EMA1(y) EMA1(z) EMA1(w)
#undef EMA1
        reinterpret_cast<float4*>(e)[i] = ee;
    }
    // scalar tail (everything when the segment is not 16-byte aligned)
    for (long i = pl.n4 * 4 + pl.first; i < pl.n; i += pl.stride) {
        const float ei = e[i];
        e[i] = ei + omd * (p[i] - ei);
    }
}

// a <-> b, bit for bit (moved as integers: no float operation touches the values).
__global__ __launch_bounds__(256) void ema_swap_kernel(EmaSegs sg) {
    const EmaPlace pl = ema_place(sg);
    unsigned* a = reinterpret_cast<unsigned*>(pl.a);
    unsigned* b = reinterpret_cast<unsigned*>(pl.b);
    for (long i = pl.first; i < pl.n4; i += pl.stride) {
        const uint4 va = reinterpret_cast<uint4*>(a)[i];
        const uint4 vb = reinterpret_cast<uint4*>(b)[i];
        reinterpret_cast<uint4*>(a)[i] = vb;
        reinterpret_cast<uint4*>(b)[i] = va;
    }
    for (long i = pl.n4 * 4 + pl.first; i < pl.n; i += pl.stride) {
        const unsigned va = a[i], vb = b[i];
        a[i] = vb;
        b[i] = va;
    }
}

// Argument checks and block placement shared by the two entry points; returns the grid size, or 0 for a bad argument.
// Grid as launch_adam sizes it: one block per 256 work items (float4 pieces, or floats in an unaligned segment), at most
// 2048 blocks in all -- above that every segment keeps one block and the rest are dealt in proportion to the work.
int ema_plan(float* const* a, const float* const* b, const long* n, int segments, EmaSegs& sg) {
    if (!a || !b || !n || segments < 1 || segments > ARCVAE_EMA_MAX_SEGMENTS) return 0;
    EmaSeg* seg[ARCVAE_EMA_MAX_SEGMENTS] = {&sg.s0, &sg.s1, &sg.s2, &sg.s3};
    long want[ARCVAE_EMA_MAX_SEGMENTS], total = 0;
    for (int i = 0; i < segments; ++i) {
        if (n[i] <= 0 || !a[i] || !b[i]) return 0;
        const uintptr_t al = reinterpret_cast<uintptr_t>(a[i]) | reinterpret_cast<uintptr_t>(b[i]);
        seg[i]->a = a[i];
        seg[i]->b = const_cast<float*>(b[i]);
        seg[i]->n = n[i];
        seg[i]->n4 = (al & 15) ? 0 : n[i] / 4;
        const long work = seg[i]->n4 > 0 ? seg[i]->n4 : n[i];
        want[i] = (work + 255) / 256;
        total += want[i];
    }
    const long cap = 2048, spare = cap - segments;
    int end = 0;
    for (int i = 0; i < ARCVAE_EMA_MAX_SEGMENTS; ++i) {
        if (i < segments) {
            const long blocks = total <= cap ? want[i] : 1 + (long)((double)spare * (double)want[i] / (double)total);
            end += (int)std::min(blocks, want[i]);
        } else {
            seg[i]->a = nullptr; seg[i]->b = nullptr; seg[i]->n = 0; seg[i]->n4 = 0;
        }
        seg[i]->end = end;
    }
    return end;
}

}  // namespace

extern "C" int arcvae_ema_update(float* const* ema, const float* const* params, const long* n, int segments,
                                 double one_minus_decay, const unsigned* guard_a, const unsigned* guard_b,
                                 hipStream_t stream) {
    if (!std::isfinite(one_minus_decay) || !(one_minus_decay > 0.0 && one_minus_decay <= 1.0)) return ARCVAE_ERR_ARG;
    EmaSegs sg;
    const int blocks = ema_plan(ema, params, n, segments, sg);
    if (blocks <= 0) return ARCVAE_ERR_ARG;
    hipLaunchKernelGGL(ema_update_kernel, dim3(blocks), dim3(256), 0, stream, sg, (float)one_minus_decay, guard_a, guard_b);
    return arcvae_launch_status();
}

extern "C" int arcvae_ema_swap(float* const* a, float* const* b, const long* n, int segments, hipStream_t stream) {
    EmaSegs sg;
    const int blocks = ema_plan(a, b, n, segments, sg);
    if (blocks <= 0) return ARCVAE_ERR_ARG;
    hipLaunchKernelGGL(ema_swap_kernel, dim3(blocks), dim3(256), 0, stream, sg);
    return arcvae_launch_status();
}
