// The dense decoder table's own functions, which every decoder of it calls: the rows' lse_T, the rows' entropy and
// cross-entropy (the per-state costs of arcvae_dec_chain_expect) and the log-likelihood of given sequences.  Contract: include/arcvae_hip.h, restated in NumPy by tests/beam_ref.py.
#include "table.h"

namespace {

// ---- lse_T of every dense row (one wave per row): lse_T = logsumexp(x * inv_temp) ----------------------------------------
__global__ __launch_bounds__(256) void table_row_lse_kernel(const float* __restrict__ logits, float* lse, long R, int V,
                                                            float inv_temp) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const float* x = logits + r * V;
    float m = -INFINITY;
    for (int w = lane; w < V; w += 64) m = fmaxf(m, x[w] * inv_temp);
    m = wave_max(m);
    float s = 0.f;
    for (int w = lane; w < V; w += 64) s += expf(x[w] * inv_temp - m);
    s = wave_sum(s);
    if (lane == 0) lse[r] = m + logf(s);
}

// ---- per-state costs of every dense row (one wave per row): h = -sum_v p lp, c = -sum_v p lq, p = expf(lp) formed once -------
// Both sums run in the same loop by the same operations (a product, a subtraction; no contraction) and the same butterfly, so a
// q that is the p table at the same lse and temperature gives c == h bit for bit.  A term whose p is 0 is skipped: its logarithm
// may be -inf.  xq NULL: h alone.
__global__ __launch_bounds__(256) void table_row_costs_kernel(const float* __restrict__ xp, const float* __restrict__ lse_p,
                                                              float inv_temp_p, const float* __restrict__ xq,
                                                              const float* __restrict__ lse_q, float inv_temp_q, float* h, float* c,
                                                              long R, int V) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const bool two = xq != nullptr;
    const float lp_row = lse_p[r], lq_row = two ? lse_q[r] : 0.f;
    float hs = 0.f, cs = 0.f;
    for (int w = lane; w < V; w += 64) {
        const float lp = table_lp(xp[r * V + w], lp_row, inv_temp_p);
        const float lq = two ? table_lp(xq[r * V + w], lq_row, inv_temp_q) : lp;
        const float p = expf(lp);
        if (p > 0.f) {
            hs -= p * lp;
            cs -= p * lq;
        }
    }
    hs = wave_sum(hs);
    cs = wave_sum(cs);
    if (lane == 0) {
        h[r] = hs;
        if (two) c[r] = cs;
    }
}

// ---- sequence log-likelihood: one wave per row, sum_{t<=e} lp(fed_t, x_t) in order, e = first end_token (T-1 if none) --------
__global__ __launch_bounds__(256) void table_seq_logprob_kernel(const float* __restrict__ logits, const float* __restrict__ lse,
                                                                const int32_t* __restrict__ x, float* out, int B, int T, int V,
                                                                int end_token, float inv_temp) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;                                   // wave-uniform
    const int32_t* xr = x + (long)b * T;
    float s = 0.f;
    bool done = false;
    for (int t0 = 0; t0 < T && !done; t0 += 64) {
        const int t = t0 + lane;
        float lp = 0.f;
        bool is_end = false;
        if (t < T) {
            const int v = min(max(xr[t], 0), V - 1);
            const int c = t == 0 ? 0 : min(max(xr[t - 1], 0), V - 1);
            const long row = (long)b * V + c;
            lp = table_lp(logits[row * V + v], lse[row], inv_temp);
            is_end = v == end_token;
        }
        const unsigned long long ends = __ballot(is_end);
        const int n = ends ? __builtin_ctzll(ends) + 1 : min(64, T - t0);
        for (int i = 0; i < n; ++i) s = s + __shfl(lp, i, 64);   // left to right, as the walks accumulate
        done = ends != 0ull;
    }
    if (lane == 0) out[b] = s;
}

}  // namespace

extern "C" int arcvae_dec_row_lse(const float* dense_logits, float* lse, long R, int V, float temperature, hipStream_t stream) {
    if (!dense_logits || !lse || R <= 0 || !table_vocab_ok(V) || !table_temp_ok(temperature, false))
        return ARCVAE_ERR_ARG;
    hipLaunchKernelGGL(table_row_lse_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, stream, dense_logits, lse, R, V,
                       1.0f / temperature);
    return arcvae_launch_status();
}

extern "C" int arcvae_dec_row_costs(const float* logits_p, const float* lse_p, float temperature_p, const float* logits_q,
                                    const float* lse_q, float temperature_q, float* h, float* c, long R, int V,
                                    hipStream_t stream) {
    if (!logits_p || !lse_p || !h || R <= 0 || !table_vocab_ok(V) || !table_temp_ok(temperature_p, true) ||
        !table_temp_ok(temperature_q, true))
        return ARCVAE_ERR_ARG;
    if ((logits_q != nullptr) != (lse_q != nullptr) || (logits_q != nullptr) != (c != nullptr)) return ARCVAE_ERR_ARG;
    hipLaunchKernelGGL(table_row_costs_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, stream, logits_p, lse_p,
                       1.0f / temperature_p, logits_q, lse_q, 1.0f / temperature_q, h, c, R, V);
    return arcvae_launch_status();
}

extern "C" int arcvae_dec_sequence_logprob(const float* dense_logits, const float* lse, const int32_t* tokens, float* out, int B,
                                           int T, int V, int end_token, float temperature, hipStream_t stream) {
    if (!dense_logits || !lse || !tokens || !out || !table_dims_ok(B, V, 1, T) || !table_temp_ok(temperature, false))
        return ARCVAE_ERR_ARG;
    hipLaunchKernelGGL(table_seq_logprob_kernel, dim3(ceil_div(B, 4)), dim3(256), 0, stream, dense_logits, lse, tokens, out, B, T,
                       V, end_token, 1.0f / temperature);
    return arcvae_launch_status();
}
