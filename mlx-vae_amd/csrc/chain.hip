// Exact MAP decoding (Viterbi) and exact chain marginals (forward recursion) over the dense decoder table -- an EXTENSION with no
// reference behaviour to match (the reference's sampler is the greedy walk, models/decoder_sampling.py:48-128).
//
// Given its conditions, a batch row's generator is a first-order Markov chain over at most 256 tokens, and rows b*V .. b*V+V-1
// of the dense table are its transition matrix.  Table, step term lp and prefix score fl(s + lp): the common contract of
// include/arcvae_hip.h (table.h), which also states both entry points' contract; tests/chain_ref.py restates it in NumPy.
//
// Kernels: one 256-thread workgroup per batch row.  The u range of a step's V x V products is cut into P contiguous parts of S
// tokens (S a multiple of 4); thread (p, v) scans part p of column v, in ascending u, against the previous step's vector in LDS
// (read four u at a time), and the threads of part 0 merge the P partial results in ascending p.  For the maximum that keeps
// "the lowest u wins a tie" (a strict > in both passes); for the sum it fixes the summation order.  Two barriers per step
// (one when P = 1); the vector is double-buffered.  The row's V x V step terms (Viterbi) or probabilities (marginals) are
// computed once into LDS when V <= CHAIN_STAGE_V and read from the table through L2 otherwise.  The end token never continues:
// its entry of the vector is -inf (maximum) or 0 (sum), as are the entries that pad V to a multiple of 4, so neither needs a
// branch in the scan.
//   viterbi    back pointers go to the caller's scratch as bytes [B, max_len, V]; the back-trace stages them through LDS in
//              chunks of CHAIN_TRACE_BYTES and one thread follows them.
//   marginals  writes alive[b, t, :] every step.
//   expect     the marginals kernel with a pack of extra arguments (ChainExpect): alive stays in registers and LDS, the columns'
//              owners keep running sums over the steps, and one block reduction after the last step forms the expectations; the
//              plain instantiation has an empty pack and none of that code.  No LDS is added.
//   viterbi_norm   the same kernel with a pack of extra arguments (ChainNorm): the end column's owner divides e_t by the length's
//              divisor and compares keys, and stores e_t to the profile where asked; the plain instantiation has an empty pack
//              and none of that code.
//   viterbi_trace  a kernel of its own, one workgroup per row: the back-trace alone, from the end token at a given length.
#include "table.h"

namespace {

constexpr int CHAIN_THREADS = 256;
constexpr int CHAIN_STAGE_V = 96;           // largest V whose V x V table is staged (36 KB: three workgroups per CU; V 80: five)
constexpr int CHAIN_TRACE_BYTES = 8192;     // back pointers staged per chunk of the back-trace (>= 32 steps at V 256)
constexpr int CHAIN_MAX_COST = 4;           // per-state costs a launch of the expectations takes
// LDS (floats): vector A [256] | vector B [256] | partial results [256] x 2 (Viterbi: value and argument; the sum uses 256) |
// lse [256] | control [4] (int / float) | table, or the back-trace's chunk
constexpr int CHAIN_OFF_B = 256, CHAIN_OFF_PV = 512, CHAIN_OFF_LSE = 1024, CHAIN_OFF_CTL = 1280,
              CHAIN_OFF_TAB = 1284;

struct ChainPlan {
    int S, P;          // tokens per part, parts: (P - 1) * S < V <= P * S, P * V <= CHAIN_THREADS
    bool staged;
    unsigned lds;      // dynamic LDS bytes
};

ChainPlan chain_plan(int V, bool trace) {
    ChainPlan p;
    int S = ceil_div(V, CHAIN_THREADS / V);
    S = (S + 3) & ~3;
    if (S < 8) S = 8;                      // shorter parts cost more in the merge than they save in the scan
    p.S = S;
    p.P = ceil_div(V, S);
    p.staged = V <= CHAIN_STAGE_V;
    const int V4 = (V + 3) & ~3;
    unsigned tail = p.staged ? (unsigned)(V4 * V * 4) : 0u;
    if (trace && tail < (unsigned)CHAIN_TRACE_BYTES) tail = CHAIN_TRACE_BYTES;
    p.lds = CHAIN_OFF_TAB * 4 + tail;
    return p;
}

// The row's lse into LDS, and (STAGED) its table: lp, or expf(lp) for the sum; rows V .. V4-1 are zero.
template <bool STAGED, bool EXP>
__device__ __forceinline__ void chain_stage(const float* __restrict__ x, const float* __restrict__ lse, float* ls, float* tab, int V,
                                            float inv_temp) {
    const int tid = threadIdx.x;
    if (tid < V) ls[tid] = lse[tid];
    __syncthreads();
    if (STAGED) {
        const int V4 = (V + 3) & ~3;
        for (int i = tid; i < V4 * V; i += CHAIN_THREADS) {
            float lp = 0.f;
            if (i < V * V) {
                lp = table_lp(x[i], ls[i / V], inv_temp);
                if (EXP) lp = expf(lp);
            }
            tab[i] = lp;
        }
        __syncthreads();
    }
}

// Step term of (u, v); u in [V, V4) reads a row that exists (its vector entry is -inf or 0).
template <bool STAGED, bool EXP>
__device__ __forceinline__ float chain_term(const float* tab, const float* __restrict__ x, const float* ls, int u, int v, int V,
                                            float inv_temp) {
    if (STAGED) return tab[u * V + v];
    const int r = min(u, V - 1);
    const float lp = table_lp(x[(long)r * V + v], ls[r], inv_temp);
    return EXP ? expf(lp) : lp;
}

// Four consecutive entries of the previous step's vector (u a multiple of 4) and their step terms into column v.
struct ChainQuad {
    float4 a;
    float t0, t1, t2, t3;
};
template <bool STAGED, bool EXP>
__device__ __forceinline__ ChainQuad chain_quad(const float* cur, const float* tab, const float* __restrict__ x, const float* ls,
                                                int u, int v, int V, float inv_temp) {
    ChainQuad q;
    q.a = *(const float4*)(cur + u);
    q.t0 = chain_term<STAGED, EXP>(tab, x, ls, u, v, V, inv_temp);
    q.t1 = chain_term<STAGED, EXP>(tab, x, ls, u + 1, v, V, inv_temp);
    q.t2 = chain_term<STAGED, EXP>(tab, x, ls, u + 2, v, V, inv_temp);
    q.t3 = chain_term<STAGED, EXP>(tab, x, ls, u + 3, v, V, inv_temp);
    return q;
}

// ---- Viterbi -----------------------------------------------------------------------------------------------------------------
// back-trace: x_{t-1} = bp[t][x_t] for t = n-1 .. 1 from x_{n-1} = tok, the rows [c0, top) of a chunk staged in LDS; whole
// workgroup, n uniform; thread 0 follows the pointers (clamped: a row outside the contract stays inside [0, V)).
__device__ __forceinline__ void chain_backtrace(uint8_t* stage, const uint8_t* bpb, int32_t* out, int n, int tok, int V) {
    const int tid = threadIdx.x;
    const int rows = CHAIN_TRACE_BYTES / V;
    for (int top = n; top > 1; top -= rows) {
        const int c0 = max(1, top - rows), nb = (top - c0) * V;
        for (int i = tid; i < nb; i += CHAIN_THREADS) stage[i] = bpb[(long)c0 * V + i];
        __syncthreads();
        if (tid == 0) {
            for (int t = top - 1; t >= c0; --t) {
                tok = min((int)stage[(t - c0) * V + tok], V - 1);
                out[t - 1] = tok;
            }
        }
        __syncthreads();
    }
}

// What the length-normalised selection adds to the kernel's arguments: the divisors (NULL = all ones) and its further outputs.
struct ChainNorm {
    const float* len_div;      // [max_len], entry n-1 divides the raw score of a sequence of length n
    float* raw_score;          // [B]
    float* by_length;          // [B, max_len] or NULL: e_t of every step
    float* open_score;         // [B] or NULL: the open candidate's raw score
};

// NormArgs: empty (arcvae_dec_viterbi) or one ChainNorm (arcvae_dec_viterbi_norm).
template <bool STAGED, class... NormArgs>
__global__ __launch_bounds__(CHAIN_THREADS) void chain_viterbi_kernel(const float* __restrict__ logits,
                                                                      const float* __restrict__ lse, uint8_t* bp, int32_t* tokens,
                                                                      float* score, int32_t* length, int V, int S, int P,
                                                                      int max_len, int min_len, int end_token, int pad_token,
                                                                      float inv_temp, NormArgs... norm_args) {
    constexpr bool NORM = sizeof...(NormArgs) > 0;
    const ChainNorm na = table_optional<ChainNorm>(norm_args...);
    extern __shared__ __align__(16) float smem[];
    float* cur = smem;
    float* nxt = smem + CHAIN_OFF_B;
    unsigned long long* pp = (unsigned long long*)(smem + CHAIN_OFF_PV);   // a part's maximum (low word) and argument, per column
    float* ls = smem + CHAIN_OFF_LSE;
    int* ctl = (int*)(smem + CHAIN_OFF_CTL);
    float* tab = smem + CHAIN_OFF_TAB;
    uint8_t* stage = (uint8_t*)tab;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int p = tid / V, v = tid - p * V;
    const bool active = p < P, owner = p == 0;               // owner: thread v of part 0 holds column v's merged result
    const int V4 = (V + 3) & ~3;
    const int lo = p * S, hi = min(lo + S, V4);
    const float* x = logits + (long)b * V * V;
    uint8_t* bpb = bp + (long)b * max_len * V;
    int32_t* out = tokens + (long)b * max_len;

    chain_stage<STAGED, false>(x, lse + (long)b * V, ls, tab, V, inv_temp);
    cur[tid] = -INFINITY;                                     // (the pads V .. V4-1 stay -inf in both vectors)
    nxt[tid] = -INFINITY;
    __syncthreads();
    // the best end candidate so far, kept by the end token's owner: e_t of the earliest t that attains the maximum
    // (NORM: res is the KEY fl(e_t / d[t]) and raw the e_t it came from)
    float res = 0.f, raw = 0.f;
    int res_t = 0;
    bool have = false;
    if (owner) {
        const float s = 0.f + chain_term<STAGED, false>(tab, x, ls, 0, v, V, inv_temp);
        if (v == end_token) {
            if (NORM) {
                if (na.by_length) na.by_length[(long)b * max_len] = s;
                if (min_len == 0) { res = s / (na.len_div ? na.len_div[0] : 1.0f); raw = s; have = true; }
            } else if (min_len == 0) { res = s; have = true; }
        } else {
            cur[v] = s;
        }
    }
    __syncthreads();
    for (int t = 1; t < max_len; ++t) {
        float best = -INFINITY;
        int arg = min(lo, V - 1);
        float div = 1.0f;                                         // (NORM) asked for before the scan, used after it
        if (NORM && owner && v == end_token && na.len_div) div = na.len_div[t];
        if (active) {
            for (int u = lo; u < hi; u += 4) {
                const ChainQuad c = chain_quad<STAGED, false>(cur, tab, x, ls, u, v, V, inv_temp);
                const float s0 = c.a.x + c.t0, s1 = c.a.y + c.t1, s2 = c.a.z + c.t2, s3 = c.a.w + c.t3;
                if (s0 > best) { best = s0; arg = u; }
                if (s1 > best) { best = s1; arg = u + 1; }
                if (s2 > best) { best = s2; arg = u + 2; }
                if (s3 > best) { best = s3; arg = u + 3; }
            }
            if (!owner) pp[tid] = (unsigned long long)__float_as_uint(best) | ((unsigned long long)(unsigned)arg << 32);
        }
        if (P > 1) __syncthreads();
        if (owner) {
            for (int q = 1; q < P; ++q) {
                const unsigned long long e = pp[q * V + v];    // (one 8-byte read: value and argument arrive together)
                const float s = __uint_as_float((unsigned)e);
                if (s > best) { best = s; arg = (int)(e >> 32); }
            }
            bpb[(long)t * V + v] = (uint8_t)arg;
            if (v == end_token) {
                if (NORM) {
                    if (na.by_length) na.by_length[(long)b * max_len + t] = best;
                    const float key = best / div;                 // one IEEE division
                    if (t >= min_len && (!have || key > res)) { res = key; raw = best; res_t = t; have = true; }
                } else if (t >= min_len && (!have || best > res)) { res = best; res_t = t; have = true; }
            } else {
                nxt[v] = best;
            }
        }
        __syncthreads();
        float* sw = cur;
        cur = nxt;
        nxt = sw;
    }
    // the result: the end candidates (above), then a_{max_len-1}[v], v != end_token ascending; a later one wins only when
    // strictly greater.  The first candidate is taken whatever it holds, so a row outside the contract still yields tokens.
    if (owner && v == end_token) {
        ctl[0] = have;
        ctl[1] = res_t;
        ((float*)ctl)[2] = res;
        if (NORM) smem[CHAIN_OFF_PV] = raw;                      // (the partial results are dead)
    }
    __syncthreads();
    if (tid == 0) {
        bool chosen = ctl[0] != 0;
        float bs = chosen ? ((float*)ctl)[2] : -INFINITY;
        int n = chosen ? ctl[1] + 1 : max_len, last = chosen ? end_token : 0;
        if (NORM) {
            // ONE open candidate: the maximum raw a_{max_len-1}[v], v != end_token, the lowest v of a tie; compared by key
            float braw = chosen ? smem[CHAIN_OFF_PV] : -INFINITY, os = -INFINITY;
            int ow = 0;
            bool any = false;
            for (int w = 0; w < V; ++w) {
                if (w == end_token) continue;
                const float s = cur[w];
                if (!any || s > os) { os = s; ow = w; any = true; }
            }
            const float ok = os / (na.len_div ? na.len_div[max_len - 1] : 1.0f);
            if (!chosen || ok > bs) { bs = ok; braw = os; n = max_len; last = ow; }
            na.raw_score[b] = braw;
            if (na.open_score) na.open_score[b] = os;
        } else {
            for (int w = 0; w < V; ++w) {
                if (w == end_token) continue;
                const float s = cur[w];
                if (!chosen || s > bs) { bs = s; n = max_len; last = w; chosen = true; }
            }
        }
        score[b] = bs;
        length[b] = n;
        out[n - 1] = last;
        ctl[1] = n;
        ctl[3] = last;
    }
    __syncthreads();
    const int n = ctl[1];
    for (int t = n + tid; t < max_len; t += CHAIN_THREADS) out[t] = pad_token;
    chain_backtrace(stage, bpb, out, n, ctl[3], V);          // (the table is dead)
}

// The sequence that ends with end_token at position n-1 (n = lengths[b] clamped into [0, max_len]), followed back through the
// pointers a Viterbi launch left in bp; pad_token after it.  One workgroup per row; LDS: one chunk of the back-trace.
__global__ __launch_bounds__(CHAIN_THREADS) void chain_trace_kernel(const uint8_t* __restrict__ bp,
                                                                    const int32_t* __restrict__ lengths, int32_t* tokens, int V,
                                                                    int max_len, int end_token, int pad_token) {
    extern __shared__ __align__(16) float smem[];
    const int tid = threadIdx.x, b = blockIdx.x;
    int32_t* out = tokens + (long)b * max_len;
    const int n = min(max(lengths[b], 0), max_len);
    for (int t = n + tid; t < max_len; t += CHAIN_THREADS) out[t] = pad_token;
    if (n > 0 && tid == 0) out[n - 1] = end_token;
    chain_backtrace((uint8_t*)smem, bp + (long)b * max_len * V, out, n, end_token, V);
}

// ---- forward recursion -------------------------------------------------------------------------------------------------------
// What the expectations add to the kernel's arguments (arcvae_dec_chain_expect): the per-state costs and the outputs, each NULL
// where not asked for.
struct ChainExpect {
    const float* cost;         // [n_cost, B*V]
    float* totals;             // [B, n_cost]
    float* visits;             // [B, V] or NULL
    float* open_mass;          // [B] or NULL
    int n_cost;                // 0 .. CHAIN_MAX_COST
    int B;
};

// ExpectArgs: empty (arcvae_dec_chain_marginals: alive[b, t, :] goes to memory every step) or one ChainExpect
// (arcvae_dec_chain_expect: alive is NULL and nothing is written per step; column v's owner keeps visits[v] = the sum of
// alive[t][v] over all steps and cont[v] = the same over the steps whose tokens are fed back, 0 .. max_len-2 and v != end_token,
// each added in step order; after the last step the workgroup reduces open_mass and the cost totals in one fixed order:
// a butterfly per wave, the four waves' results through the dead partial-result area, added in ascending wave order).
template <bool STAGED, class... ExpectArgs>
__global__ __launch_bounds__(CHAIN_THREADS) void chain_marginals_kernel(const float* __restrict__ logits,
                                                                        const float* __restrict__ lse, float* alive, int V, int S,
                                                                        int P, int max_len, int end_token, float inv_temp,
                                                                        ExpectArgs... expect_args) {
    constexpr bool EXPECT = sizeof...(ExpectArgs) > 0;
    const ChainExpect ea = table_optional<ChainExpect>(expect_args...);
    extern __shared__ __align__(16) float smem[];
    float* cur = smem;
    float* nxt = smem + CHAIN_OFF_B;
    float* pv = smem + CHAIN_OFF_PV;
    float* ls = smem + CHAIN_OFF_LSE;
    float* tab = smem + CHAIN_OFF_TAB;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int p = tid / V, v = tid - p * V;
    const bool active = p < P, owner = p == 0;
    const int V4 = (V + 3) & ~3;
    const int lo = p * S, hi = min(lo + S, V4);
    const float* x = logits + (long)b * V * V;
    float* ob = alive + (long)b * max_len * V;

    chain_stage<STAGED, true>(x, lse + (long)b * V, ls, tab, V, inv_temp);
    cur[tid] = 0.f;                                           // (the pads V .. V4-1 and the end token stay 0 in both vectors)
    nxt[tid] = 0.f;
    __syncthreads();
    float vis = 0.f, cont = 0.f, last = 0.f;                  // (EXPECT) the owner's sums and its alive[max_len-1][v]
    if (owner) {
        const float s = chain_term<STAGED, true>(tab, x, ls, 0, v, V, inv_temp);
        if (EXPECT) {
            vis = s;
            last = s;
            if (v != end_token && max_len > 1) cont = s;
        } else {
            ob[v] = s;
        }
        if (v != end_token) cur[v] = s;
    }
    __syncthreads();
    for (int t = 1; t < max_len; ++t) {
        float acc = 0.f;
        if (active) {
            for (int u = lo; u < hi; u += 4) {
                const ChainQuad c = chain_quad<STAGED, true>(cur, tab, x, ls, u, v, V, inv_temp);
                acc = fmaf(c.a.x, c.t0, acc);
                acc = fmaf(c.a.y, c.t1, acc);
                acc = fmaf(c.a.z, c.t2, acc);
                acc = fmaf(c.a.w, c.t3, acc);
            }
            if (!owner) pv[tid] = acc;
        }
        if (P > 1) __syncthreads();
        if (owner) {
            for (int q = 1; q < P; ++q) acc += pv[q * V + v];
            if (EXPECT) {
                vis += acc;
                last = acc;
                if (v != end_token && t + 1 < max_len) cont += acc;
            } else {
                ob[(long)t * V + v] = acc;
            }
            if (v != end_token) nxt[v] = acc;
        }
        __syncthreads();
        float* sw = cur;
        cur = nxt;
        nxt = sw;
    }
    if (EXPECT) {
        // (the loop's last barrier is behind every read of the partial results: the area is dead)
        if (owner && ea.visits) ea.visits[(long)b * V + v] = vis;
        float part[CHAIN_MAX_COST + 1];                       // open_mass, then the totals: every thread takes part, with 0
        part[0] = owner && v != end_token ? last : 0.f;
#pragma unroll
        for (int k = 0; k < CHAIN_MAX_COST; ++k) {
            float r = 0.f;
            // a state that is never fed back costs nothing, whatever its cost holds (0 * inf is not relied on)
            if (k < ea.n_cost && owner && cont > 0.f) r = ea.cost[((long)k * ea.B + b) * V + v] * cont;
            part[k + 1] = r;
        }
#pragma unroll
        for (int k = 0; k <= CHAIN_MAX_COST; ++k) {
            if (k > ea.n_cost) break;                         // (uniform)
            const float w = wave_sum(part[k]);
            if ((tid & 63) == 0) pv[(tid >> 6) * (CHAIN_MAX_COST + 1) + k] = w;
        }
        __syncthreads();
        if (tid <= ea.n_cost) {
            float s = pv[tid];
            for (int w = 1; w < CHAIN_THREADS / 64; ++w) s += pv[w * (CHAIN_MAX_COST + 1) + tid];
            if (tid == 0) {
                if (ea.open_mass) ea.open_mass[b] = s;
            } else {
                const int k = tid - 1;
                ea.totals[(long)b * ea.n_cost + k] = ea.cost[((long)k * ea.B + b) * V] + s;      // the start row always counts
            }
        }
    }
}

bool chain_args_ok(const void* logits, const void* lse, int B, int V, int max_len, int end_token, float temperature) {
    return logits && lse && table_dims_ok(B, V, 1, max_len) && table_end_ok(end_token, V) && table_temp_ok(temperature, true);
}

}  // namespace

extern "C" int arcvae_dec_viterbi_ws_bytes(int B, int V, int max_len, long* bytes) {
    if (!bytes || !table_dims_ok(B, V, 1, max_len)) return ARCVAE_ERR_ARG;
    *bytes = (long)B * max_len * V;
    return ARCVAE_OK;
}

extern "C" int arcvae_dec_viterbi(const float* dense_logits, const float* lse, int32_t* tokens, float* score, int32_t* length,
                                  void* ws, long ws_bytes, int B, int V, int max_len, int min_len, int end_token, int pad_token,
                                  float temperature, hipStream_t stream) {
    if (!chain_args_ok(dense_logits, lse, B, V, max_len, end_token, temperature)) return ARCVAE_ERR_ARG;
    if (!tokens || !score || !length || !ws || !table_min_len_ok(min_len, max_len) || !table_pad_ok(pad_token) ||
        ws_bytes < (long)B * max_len * V)
        return ARCVAE_ERR_ARG;
    const ChainPlan pl = chain_plan(V, true);
    const float inv_temp = 1.0f / temperature;
    if (pl.staged)
        hipLaunchKernelGGL(chain_viterbi_kernel<true>, dim3(B), dim3(CHAIN_THREADS), pl.lds, stream, dense_logits, lse, (uint8_t*)ws,
                           tokens, score, length, V, pl.S, pl.P, max_len, min_len, end_token, pad_token, inv_temp);
    else
        hipLaunchKernelGGL(chain_viterbi_kernel<false>, dim3(B), dim3(CHAIN_THREADS), pl.lds, stream, dense_logits, lse,
                           (uint8_t*)ws, tokens, score, length, V, pl.S, pl.P, max_len, min_len, end_token, pad_token, inv_temp);
    return arcvae_launch_status();
}

extern "C" int arcvae_dec_viterbi_norm(const float* dense_logits, const float* lse, const float* len_div, int32_t* tokens,
                                       float* score, float* raw_score, int32_t* length, float* by_length, float* open_score,
                                       void* ws, long ws_bytes, int B, int V, int max_len, int min_len, int end_token,
                                       int pad_token, float temperature, hipStream_t stream) {
    if (!chain_args_ok(dense_logits, lse, B, V, max_len, end_token, temperature)) return ARCVAE_ERR_ARG;
    if (!tokens || !score || !raw_score || !length || !ws || !table_min_len_ok(min_len, max_len) || !table_pad_ok(pad_token) ||
        ws_bytes < (long)B * max_len * V)
        return ARCVAE_ERR_ARG;
    const ChainPlan pl = chain_plan(V, true);
    const float inv_temp = 1.0f / temperature;
    const ChainNorm na = {len_div, raw_score, by_length, open_score};
    if (pl.staged)
        hipLaunchKernelGGL((chain_viterbi_kernel<true, ChainNorm>), dim3(B), dim3(CHAIN_THREADS), pl.lds, stream, dense_logits, lse,
                           (uint8_t*)ws, tokens, score, length, V, pl.S, pl.P, max_len, min_len, end_token, pad_token, inv_temp, na);
    else
        hipLaunchKernelGGL((chain_viterbi_kernel<false, ChainNorm>), dim3(B), dim3(CHAIN_THREADS), pl.lds, stream, dense_logits, lse,
                           (uint8_t*)ws, tokens, score, length, V, pl.S, pl.P, max_len, min_len, end_token, pad_token, inv_temp, na);
    return arcvae_launch_status();
}

extern "C" int arcvae_dec_viterbi_trace(const void* ws, long ws_bytes, const int32_t* lengths, int32_t* tokens, int B, int V,
                                        int max_len, int end_token, int pad_token, hipStream_t stream) {
    if (!ws || !lengths || !tokens || !table_dims_ok(B, V, 1, max_len) || !table_end_ok(end_token, V) || !table_pad_ok(pad_token))
        return ARCVAE_ERR_ARG;
    if (ws_bytes < (long)B * max_len * V) return ARCVAE_ERR_ARG;
    hipLaunchKernelGGL(chain_trace_kernel, dim3(B), dim3(CHAIN_THREADS), CHAIN_TRACE_BYTES, stream, (const uint8_t*)ws, lengths,
                       tokens, V, max_len, end_token, pad_token);
    return arcvae_launch_status();
}

extern "C" int arcvae_dec_chain_marginals(const float* dense_logits, const float* lse, float* alive, int B, int V, int max_len,
                                          int end_token, float temperature, hipStream_t stream) {
    if (!chain_args_ok(dense_logits, lse, B, V, max_len, end_token, temperature) || !alive) return ARCVAE_ERR_ARG;
    const ChainPlan pl = chain_plan(V, false);
    const float inv_temp = 1.0f / temperature;
    if (pl.staged)
        hipLaunchKernelGGL(chain_marginals_kernel<true>, dim3(B), dim3(CHAIN_THREADS), pl.lds, stream, dense_logits, lse, alive, V,
                           pl.S, pl.P, max_len, end_token, inv_temp);
    else
        hipLaunchKernelGGL(chain_marginals_kernel<false>, dim3(B), dim3(CHAIN_THREADS), pl.lds, stream, dense_logits, lse, alive, V,
                           pl.S, pl.P, max_len, end_token, inv_temp);
    return arcvae_launch_status();
}

extern "C" int arcvae_dec_chain_expect(const float* dense_logits, const float* lse, const float* cost, int n_cost, float* totals,
                                       float* visits, float* open_mass, int B, int V, int max_len, int end_token,
                                       float temperature, hipStream_t stream) {
    if (!chain_args_ok(dense_logits, lse, B, V, max_len, end_token, temperature)) return ARCVAE_ERR_ARG;
    if (n_cost < 0 || n_cost > CHAIN_MAX_COST || (cost != nullptr) != (n_cost > 0) || (totals != nullptr) != (n_cost > 0))
        return ARCVAE_ERR_ARG;
    if (n_cost == 0 && !visits && !open_mass) return ARCVAE_ERR_ARG;
    const ChainPlan pl = chain_plan(V, false);
    const float inv_temp = 1.0f / temperature;
    const ChainExpect ea = {cost, totals, visits, open_mass, n_cost, B};
    if (pl.staged)
        hipLaunchKernelGGL((chain_marginals_kernel<true, ChainExpect>), dim3(B), dim3(CHAIN_THREADS), pl.lds, stream, dense_logits,
                           lse, (float*)nullptr, V, pl.S, pl.P, max_len, end_token, inv_temp, ea);
    else
        hipLaunchKernelGGL((chain_marginals_kernel<false, ChainExpect>), dim3(B), dim3(CHAIN_THREADS), pl.lds, stream, dense_logits,
                           lse, (float*)nullptr, V, pl.S, pl.P, max_len, end_token, inv_temp, ea);
    return arcvae_launch_status();
}
