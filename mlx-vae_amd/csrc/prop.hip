// Property predictor head on the latent code (an extension: the reference's predictor branch cannot run).
//
//   pred = fc2(tanh(fc1(z)))        fc1: Linear(Z -> Hp), fc2: Linear(Hp -> C)
//   prop_loss = mean over B*C of (pred - cond)^2,  weighted_prop_loss = lambda_prop * prop_loss  (lambda_prop = hyper[5])
//
// Two launches per training step:
//   prop_rows_kernel   ON the chain, between arcvae_latent_loss and arcvae_enc_heads_backward: 4 rows per block; forward,
//                      per-row dpred (global B*C divisor, lambda folded in), da = dpred W2 * (1 - t^2), and dz = da W1 folded
//                      straight into d(mu_raw) / d(lv_raw) through the reparameterisation and the tanh bounds.  Leaves the
//                      per-row partials (t, da, dpred, squared error) in the caller's workspace.
//   prop_reduce_kernel OFF the chain (the engine runs it in the step's finish): per gradient element, S threads sum
//                      contiguous row slices of the per-row partials, added in slice order (S fixed by B) -- deterministic,
//                      bitwise repeatable -- and OVERWRITES the predictor's gradient (no zero fill); one more output is
//                      the loss: scalars[5] / scalars[6].
// fp32 throughout (plain FMA, libm tanhf / expf).
#include "common.h"

namespace {

constexpr int PROP_RB = 4;         // rows per block of the row kernel (bs 64: 16 blocks)
constexpr int PROP_THREADS = 256;
constexpr int PROP_MAX_Z = 512;
constexpr int PROP_MAX_HP = 256;
constexpr int PROP_MAX_C = 8;
constexpr int PROP_BATCH = 8;      // loads issued back to back before their FMAs (the chain is latency-bound)
constexpr int PROP_ROW = PROP_MAX_HP > PROP_MAX_Z ? PROP_MAX_HP : PROP_MAX_Z;   // LDS row length

__device__ __forceinline__ int pow2_floor(int x) {
    int p = 1;
    while (p * 2 <= x) p *= 2;
    return p;
}

struct PropRowsArgs {
    const float* z;
    const float* cond;     // null: forward only, no loss
    const float* eps;
    const float* mu_raw;
    const float* lv_raw;
    const float* W1;
    const float* b1;
    const float* W2;
    const float* b2;
    const float* hyper;
    float* dmu_raw;        // train: += the predictor's share
    float* dlv_raw;
    float* pred;           // optional [B, C]
    float* t_ws;           // [B, Hp]  tanh activations
    float* da_ws;          // [B, Hp]  d/d(fc1 pre-activation), lambda included
    float* g_ws;           // [B, C]   d/d(pred), lambda included
    float* sq_ws;          // [B]      sum over c of (pred - cond)^2
    int B, Z, C, Hp;
    int train;
};

// dz of row r, latent unit k, into d(mu_raw) / d(lv_raw)
__device__ __forceinline__ void prop_fold(const PropRowsArgs& a, int row, int k, float dz) {
    const long idx = (long)row * a.Z + k;
    const float tm = tanhf(a.mu_raw[idx] / 2.0f);
    const float tl = tanhf(a.lv_raw[idx] / 2.0f);
    const float lv = tl - 1.0f;
    a.dmu_raw[idx] += dz * (1.0f - tm * tm);
    a.dlv_raw[idx] += dz * a.eps[idx] * (0.5f * expf(0.5f * lv)) * (0.5f * (1.0f - tl * tl));
}

// acc[r] += sum over j in [j0, j1) of x[r][j] * w[j * stride], loads in batches of PROP_BATCH, j ascending (fixed order)
__device__ __forceinline__ void prop_dot_rows(float (&acc)[PROP_RB], const float (*x)[PROP_ROW], const float* __restrict__ w,
                                              long stride, int j0, int j1) {
    int j = j0;
    for (; j + PROP_BATCH <= j1; j += PROP_BATCH) {
        float wv[PROP_BATCH];
#pragma unroll
        for (int q = 0; q < PROP_BATCH; ++q) wv[q] = w[(long)(j + q) * stride];
#pragma unroll
        for (int q = 0; q < PROP_BATCH; ++q)
#pragma unroll
            for (int r = 0; r < PROP_RB; ++r) acc[r] = fmaf(x[r][j + q], wv[q], acc[r]);
    }
    for (; j < j1; ++j) {
        const float wv = w[(long)j * stride];
#pragma unroll
        for (int r = 0; r < PROP_RB; ++r) acc[r] = fmaf(x[r][j], wv, acc[r]);
    }
}

__global__ __launch_bounds__(PROP_THREADS) void prop_rows_kernel(PropRowsArgs a) {
    __shared__ float zs[PROP_RB][PROP_ROW];            // z rows
    __shared__ float ts[PROP_RB][PROP_ROW];            // tanh activations, then da (in place)
    __shared__ float part[PROP_RB][PROP_THREADS];      // k-slice partials of fc1, h-slice partials of dz
    __shared__ float ds[PROP_RB][PROP_MAX_C];          // pred - cond
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r0 = blockIdx.x * PROP_RB;
    const int nr = min(PROP_RB, a.B - r0);
    const int Z = a.Z, Hp = a.Hp, C = a.C;

    for (int i = tid; i < PROP_RB * Z; i += PROP_THREADS) {
        const int r = i / Z, k = i - r * Z;
        zs[r][k] = r < nr ? a.z[(long)(r0 + r) * Z + k] : 0.0f;
    }
    for (int i = tid; i < PROP_RB * Hp; i += PROP_THREADS) ts[i / Hp][i % Hp] = 0.0f;
    __syncthreads();

    // fc1: thread (h, s) forms the k-slice s of unit h for the block's rows; SL slices per unit, SL * Hp <= 256
    const int SL = pow2_floor(PROP_THREADS / Hp);
    if (tid < SL * Hp) {
        const int h = tid % Hp, s = tid / Hp;
        const int L = (Z + SL - 1) / SL;
        float acc[PROP_RB] = {};
        prop_dot_rows(acc, zs, a.W1 + (long)h * Z, 1, min(Z, s * L), min(Z, (s + 1) * L));
#pragma unroll
        for (int r = 0; r < PROP_RB; ++r) part[r][s * Hp + h] = acc[r];
    }
    __syncthreads();
    for (int i = tid; i < nr * Hp; i += PROP_THREADS) {
        const int r = i / Hp, h = i - r * Hp;
        float acc = 0.f;
        for (int s = 0; s < SL; ++s) acc += part[r][s * Hp + h];
        const float t = tanhf(acc + a.b1[h]);
        ts[r][h] = t;
        if (a.train) a.t_ws[(long)(r0 + r) * Hp + h] = t;
    }
    __syncthreads();

    // fc2: one wave per (row, property), lanes over the hidden units
    for (int p = wave; p < nr * C; p += PROP_THREADS / 64) {
        const int r = p / C, c = p - r * C;
        float acc = 0.f;
        for (int h = lane; h < Hp; h += 64) acc = fmaf(ts[r][h], a.W2[(long)c * Hp + h], acc);
        acc = wave_sum(acc);
        if (lane == 0) {
            const float pv = acc + a.b2[c];
            if (a.pred) a.pred[(long)(r0 + r) * C + c] = pv;
            if (a.cond) ds[r][c] = pv - a.cond[(long)(r0 + r) * C + c];
        }
    }
    __syncthreads();
    if (!a.cond) return;
    if (tid < nr) {
        float sq = 0.f;
        for (int c = 0; c < C; ++c) sq = fmaf(ds[tid][c], ds[tid][c], sq);
        a.sq_ws[r0 + tid] = sq;
    }
    if (!a.train) return;

    // d(lambda * mean (pred - cond)^2) / d(pred) = lambda * 2 (pred - cond) / (B C)
    const float scale = a.hyper[5] * 2.0f / ((float)a.B * (float)C);
    for (int i = tid; i < nr * C; i += PROP_THREADS) {
        const int r = i / C, c = i - r * C;
        a.g_ws[(long)(r0 + r) * C + c] = scale * ds[r][c];
    }
    // da = (dpred . W2) * (1 - t^2), in place over t (each element is read and written by the same thread)
    for (int i = tid; i < nr * Hp; i += PROP_THREADS) {
        const int r = i / Hp, h = i - r * Hp;
        float acc = 0.f;
        for (int c = 0; c < C; ++c) acc = fmaf(scale * ds[r][c], a.W2[(long)c * Hp + h], acc);
        const float t = ts[r][h];
        const float da = acc * (1.0f - t * t);
        ts[r][h] = da;
        a.da_ws[(long)(r0 + r) * Hp + h] = da;
    }
    __syncthreads();

    // dz = da . W1: thread (k, s) forms the h-slice s for latent unit k (W1 loads coalesced over k); HS * Z <= 256, or
    // HS = 1 above Z = 256
    const int HS = Z <= PROP_THREADS ? pow2_floor(PROP_THREADS / Z) : 1;
    const int HL = (Hp + HS - 1) / HS;
    for (int i = tid; i < HS * Z; i += PROP_THREADS) {
        const int s = i / Z, k = i - s * Z;
        float acc[PROP_RB] = {};
        prop_dot_rows(acc, ts, a.W1 + k, Z, min(Hp, s * HL), min(Hp, (s + 1) * HL));
        if (HS == 1) {
            for (int r = 0; r < nr; ++r) prop_fold(a, r0 + r, k, acc[r]);
        } else {
#pragma unroll
            for (int r = 0; r < PROP_RB; ++r) part[r][s * Z + k] = acc[r];
        }
    }
    if (HS == 1) return;
    __syncthreads();
    for (int i = tid; i < nr * Z; i += PROP_THREADS) {
        const int r = i / Z, k = i - r * Z;
        float dz = 0.f;
        for (int s = 0; s < HS; ++s) dz += part[r][s * Z + k];
        prop_fold(a, r0 + r, k, dz);
    }
}

struct PropReduceArgs {
    const float* z;
    const float* t_ws;
    const float* da_ws;
    const float* g_ws;
    const float* sq_ws;
    const float* hyper;
    float* dW1;            // null: loss scalars only
    float* db1;
    float* dW2;
    float* db2;
    float* scalars;        // null: gradients only
    int B, Z, C, Hp;
};

// sum over r in [r0, r1) of term(r), ascending; the terms' loads are issued PROP_BATCH at a time
template <class F>
__device__ __forceinline__ float prop_row_sum(int r0, int r1, F term) {
    float acc = 0.f;
    int r = r0;
    for (; r + PROP_BATCH <= r1; r += PROP_BATCH) {
        float v[PROP_BATCH];
#pragma unroll
        for (int q = 0; q < PROP_BATCH; ++q) v[q] = term(r + q);
#pragma unroll
        for (int q = 0; q < PROP_BATCH; ++q) acc += v[q];
    }
    for (; r < r1; ++r) acc += term(r);
    return acc;
}

// Output i of the reduction -> its kind (0 dW1, 1 db1, 2 dW2, 3 db2, 4 the loss) and its index j within that tensor.
__device__ __forceinline__ int prop_out_kind(const PropReduceArgs& a, long i, long& j) {
    j = i;
    if (a.dW1) {
        const long n[4] = {(long)a.Hp * a.Z, a.Hp, (long)a.C * a.Hp, a.C};
        for (int kind = 0; kind < 4; ++kind) {
            if (j < n[kind]) return kind;
            j -= n[kind];
        }
    }
    return 4;
}

__device__ __forceinline__ float prop_out_rows(const PropReduceArgs& a, int kind, long j, int r0, int r1) {
    const int Z = a.Z, C = a.C, Hp = a.Hp;
    const float* __restrict__ da = a.da_ws;
    const float* __restrict__ t = a.t_ws;
    const float* __restrict__ g = a.g_ws;
    const float* __restrict__ z = a.z;
    const float* __restrict__ sq = a.sq_ws;
    switch (kind) {
    case 0: {
        const int h = (int)(j / Z), k = (int)(j - (long)h * Z);
        return prop_row_sum(r0, r1, [&](int r) { return da[(long)r * Hp + h] * z[(long)r * Z + k]; });
    }
    case 1: return prop_row_sum(r0, r1, [&](int r) { return da[(long)r * Hp + j]; });
    case 2: {
        const int c = (int)(j / Hp), h = (int)(j - (long)c * Hp);
        return prop_row_sum(r0, r1, [&](int r) { return g[(long)r * C + c] * t[(long)r * Hp + h]; });
    }
    case 3: return prop_row_sum(r0, r1, [&](int r) { return g[(long)r * C + j]; });
    default: return prop_row_sum(r0, r1, [&](int r) { return sq[r]; });
    }
}

// A block holds 256 / S outputs; each output's rows are split into S contiguous slices (S = 1 at bs <= 127, 16 from bs 1024
// on: prop_reduce_slices), each thread sums one slice in row order, and the slices are added in slice order -- the order
// depends on B alone, so the result is bitwise repeatable.
__global__ __launch_bounds__(PROP_THREADS) void prop_reduce_kernel(PropReduceArgs a, long items, int S) {
    __shared__ float part[PROP_THREADS];
    const int O = PROP_THREADS / S;
    const int o = threadIdx.x % O, s = threadIdx.x / O;
    const long i = (long)blockIdx.x * O + o;
    const int RL = (a.B + S - 1) / S;
    const int r0 = min(a.B, s * RL), r1 = min(a.B, (s + 1) * RL);
    long j = 0;
    const int kind = i < items ? prop_out_kind(a, i, j) : -1;
    part[threadIdx.x] = kind >= 0 ? prop_out_rows(a, kind, j, r0, r1) : 0.0f;
    __syncthreads();
    if (s != 0 || kind < 0) return;
    float v = 0.f;
    for (int q = 0; q < S; ++q) v += part[q * O + o];
    switch (kind) {
    case 0: a.dW1[j] = v; break;
    case 1: a.db1[j] = v; break;
    case 2: a.dW2[j] = v; break;
    case 3: a.db2[j] = v; break;
    default: {
        const float p = v / ((float)a.B * (float)a.C);
        a.scalars[5] = p;
        a.scalars[6] = a.hyper[5] * p;
    }
    }
}

// row slices per output of prop_reduce_kernel: a power of two in [1, 16], about 64 rows or more per slice
int prop_reduce_slices(int B) {
    int S = 1;
    while (S < 16 && B / (2 * S) >= 64) S *= 2;
    return S;
}

long prop_ws_need(int B, int C, int Hp) { return (long)B * (2L * Hp + C + 1); }

bool prop_dims_ok(int B, int Z, int C, int Hp) {
    return B >= 1 && B <= (1 << 24) && Z >= 1 && Z <= PROP_MAX_Z && C >= 1 && C <= PROP_MAX_C && Hp >= 1 &&
           Hp <= PROP_MAX_HP;
}

void prop_ws_split(float* ws, int B, int C, int Hp, float** t, float** da, float** g, float** sq) {
    *t = ws;
    *da = ws + (long)B * Hp;
    *g = ws + 2L * B * Hp;
    *sq = ws + 2L * B * Hp + (long)B * C;
}

int prop_reduce_launch(const float* z, float* ws, const float* hyper, float* dW1, float* db1, float* dW2, float* db2,
                       float* scalars, int B, int Z, int C, int Hp, hipStream_t stream) {
    PropReduceArgs r{};
    float *t, *da, *g, *sq;
    prop_ws_split(ws, B, C, Hp, &t, &da, &g, &sq);
    r.z = z; r.t_ws = t; r.da_ws = da; r.g_ws = g; r.sq_ws = sq; r.hyper = hyper;
    r.dW1 = dW1; r.db1 = db1; r.dW2 = dW2; r.db2 = db2; r.scalars = scalars;
    r.B = B; r.Z = Z; r.C = C; r.Hp = Hp;
    const long items = (dW1 ? (long)Hp * Z + Hp + (long)C * Hp + C : 0) + (scalars ? 1 : 0);
    const int S = prop_reduce_slices(B), O = PROP_THREADS / S;
    hipLaunchKernelGGL(prop_reduce_kernel, dim3((unsigned)((items + O - 1) / O)), dim3(PROP_THREADS), 0, stream, r, items, S);
    return arcvae_launch_status();
}

}  // namespace

extern "C" int arcvae_prop_ws_floats(int B, int Z, int C, int Hp, long* floats) {
    if (!floats || !prop_dims_ok(B, Z, C, Hp)) return ARCVAE_ERR_ARG;
    *floats = prop_ws_need(B, C, Hp);
    return ARCVAE_OK;
}

extern "C" int arcvae_prop_forward(const float* z, const float* cond, const float* W1, const float* b1, const float* W2,
                                   const float* b2, const float* hyper, float* pred, float* scalars, float* ws,
                                   long ws_floats, int B, int Z, int C, int Hp, hipStream_t stream) {
    if (!prop_dims_ok(B, Z, C, Hp) || !z || !W1 || !b1 || !W2 || !b2) return ARCVAE_ERR_ARG;
    if (!pred && !scalars) return ARCVAE_ERR_ARG;                  // nothing to compute
    if (scalars && (!cond || !hyper || !ws || ws_floats < prop_ws_need(B, C, Hp))) return ARCVAE_ERR_ARG;
    PropRowsArgs a{};
    a.z = z; a.cond = scalars ? cond : nullptr; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2; a.hyper = hyper;
    a.pred = pred;
    if (scalars) {
        float *t, *da, *g, *sq;
        prop_ws_split(ws, B, C, Hp, &t, &da, &g, &sq);
        a.sq_ws = sq;
    }
    a.B = B; a.Z = Z; a.C = C; a.Hp = Hp; a.train = 0;
    hipLaunchKernelGGL(prop_rows_kernel, dim3(ceil_div(B, PROP_RB)), dim3(PROP_THREADS), 0, stream, a);
    int rc = arcvae_launch_status();
    if (rc || !scalars) return rc;
    return prop_reduce_launch(z, ws, hyper, nullptr, nullptr, nullptr, nullptr, scalars, B, Z, C, Hp, stream);
}

extern "C" int arcvae_prop_backward(const float* z, const float* cond, const float* eps, const float* mu_raw,
                                    const float* lv_raw, const float* W1, const float* b1, const float* W2, const float* b2,
                                    const float* hyper, float* dmu_raw, float* dlv_raw, float* pred, float* ws,
                                    long ws_floats, int B, int Z, int C, int Hp, hipStream_t stream) {
    if (!prop_dims_ok(B, Z, C, Hp)) return ARCVAE_ERR_ARG;
    if (!z || !cond || !eps || !mu_raw || !lv_raw || !W1 || !b1 || !W2 || !b2 || !hyper || !dmu_raw || !dlv_raw || !ws)
        return ARCVAE_ERR_ARG;
    if (ws_floats < prop_ws_need(B, C, Hp)) return ARCVAE_ERR_ARG;
    PropRowsArgs a{};
    a.z = z; a.cond = cond; a.eps = eps; a.mu_raw = mu_raw; a.lv_raw = lv_raw;
    a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2; a.hyper = hyper;
    a.dmu_raw = dmu_raw; a.dlv_raw = dlv_raw; a.pred = pred;
    prop_ws_split(ws, B, C, Hp, &a.t_ws, &a.da_ws, &a.g_ws, &a.sq_ws);
    a.B = B; a.Z = Z; a.C = C; a.Hp = Hp; a.train = 1;
    hipLaunchKernelGGL(prop_rows_kernel, dim3(ceil_div(B, PROP_RB)), dim3(PROP_THREADS), 0, stream, a);
    return arcvae_launch_status();
}

extern "C" int arcvae_prop_wgrad(const float* z, const float* ws, long ws_floats, const float* hyper, float* dW1,
                                 float* db1, float* dW2, float* db2, float* scalars, int B, int Z, int C, int Hp,
                                 hipStream_t stream) {
    if (!prop_dims_ok(B, Z, C, Hp)) return ARCVAE_ERR_ARG;
    if (!z || !ws || !hyper || !dW1 || !db1 || !dW2 || !db2 || !scalars) return ARCVAE_ERR_ARG;
    if (ws_floats < prop_ws_need(B, C, Hp)) return ARCVAE_ERR_ARG;
    return prop_reduce_launch(z, const_cast<float*>(ws), hyper, dW1, db1, dW2, db2, scalars, B, Z, C, Hp, stream);
}
