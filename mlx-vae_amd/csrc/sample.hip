// Top-k / nucleus (top-p) truncated sampling over the dense decoder table -- an EXTENSION with no reference behaviour to match
// (the reference's sampler is the greedy walk, models/decoder_sampling.py:48-128).  Contract: include/arcvae_hip.h, restated in
// NumPy by tests/topkp_ref.py; table and seed as the common contract there (table.h).
//
// One device function, topkp_row, truncates a table row: one wave, a lane holds the four entries j = 4*lane + e, exactly as the
// categorical walk (decoder.hip).
//   1. s_j = fl(x_j * inv_temp); key_j = ordered_key(s_j) << 8 | (255 - j) (table.h): unique, and descending key
//      order is the contract's order (s descending, then token ascending; -0 is folded into +0 first, as s compares them equal).
//   2. a bitonic sort of the 256 keys, descending, across the wave: position p = 4*lane + e; partners at distance 1 and 2 are
//      in the lane, the others one __shfl_xor away.  Padding entries (j >= V) hold key 0 and sort behind every real one.
//   3. e_p = expf(s_p - s_0) for p < |K| = min(k, V), 0 beyond; C = inclusive scan in sorted order (in-lane, then across lanes).
//   4. n = the first position p >= 1 of K that fails the nucleus test fl(C_p - e_p) < fl(p * M_K) (|K| if none).
// Placement: a pre-pass truncates all B*V rows once, in parallel (topkp_rows_kernel<true>: count, the |K| cumulative masses and
// tokens of each row into the caller's workspace), and the walk (one wave per batch row) only reads those lists.  Truncating
// inside the walk instead, for the B * max_len rows it visits, was measured at 0.42 / 0.67 ms per bs-1024 batch (max_length
// 80 / 128, V 80) against 0.23 / 0.27 ms for pre-pass + walk: one wave per SIMD has nothing to hide the sort's latency
// (DESIGN.md section 10).  The pre-pass and the materialising entry point run the same topkp_row, so the walk's decisions are
// those of the inspected rows, bit for bit.
// Min-p, locally typical and minimum-length sampling (arcvae_dec_trunc_rows / arcvae_dec_sample_chain_trunc; restated by
// tests/trunc_ref.py) write the same lists by other rules (trunc_row) and walk them with the same kernel: min_len > 0 is a second
// list set, built with the end token banned, which the steps t < min_len read.
#include "table.h"

namespace {

__device__ __forceinline__ unsigned long long topkp_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned long long topkp_min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

// element e (wave-uniform) of a lane's four values, without a dynamically indexed array (which would live in scratch)
template <typename T>
__device__ __forceinline__ T topkp_pick4(const T (&v)[4], int e) {
    return e == 0 ? v[0] : (e == 1 ? v[1] : (e == 2 ? v[2] : v[3]));
}

// Position p = 4*lane + e of the wave's 256 keys: descending bitonic sort (blocks of size k alternate direction; the last
// stage, k = 256, is one descending block).  Keys are unique, so min / max pick one element of each pair.
__device__ __forceinline__ void topkp_sort(unsigned long long (&key)[4], int lane) {
#pragma unroll
    for (int k = 2; k <= TABLE_MAX_V; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            unsigned long long other[4];
            if (j >= 4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) other[e] = __shfl_xor(key[e], j >> 2, 64);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) other[e] = key[e ^ j];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int p = 4 * lane + e;
                const bool desc = (p & k) == 0, lower = (p & j) == 0;
                key[e] = (lower == desc) ? topkp_max(key[e], other[e]) : topkp_min(key[e], other[e]);
            }
        }
    }
}

// The truncated distribution of one table row (wave-wide; every output is per lane for positions 4*lane + e, n and c_last are
// wave-uniform): tok = the whole order (positions < V), cum = C (positions < |K|; 0 beyond), n = |P|.
__device__ __forceinline__ void topkp_row(const float* __restrict__ row, int V, float inv_temp, int K, float top_p, int lane,
                                          int (&tok)[4], float (&cum)[4], int& n) {
    unsigned long long key[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int j = 4 * lane + e;
        key[e] = 0ull;
        if (j < V) {
            float s = table_scaled(row[j], inv_temp);
            if (s == 0.f) s = 0.f;                       // -0 folded into +0: one key, the tie goes to the token index
            key[e] = ((unsigned long long)ordered_key(s) << 8) | (unsigned long long)(255 - j);
        }
    }
    topkp_sort(key, lane);
    float s[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        tok[e] = 255 - (int)(key[e] & 255ull);
        s[e] = ordered_value((unsigned)(key[e] >> 8));
    }
    const float m = __shfl(s[0], 0, 64);                  // position 0: the row's largest s
    float ev[4], c[4], run = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        ev[e] = 4 * lane + e < K ? expf(s[e] - m) : 0.f;
        run += ev[e];
        c[e] = run;
    }
    float incl = run;                                     // inclusive scan of the lanes' totals
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    float before = __shfl_up(incl, 1, 64);
    if (lane == 0) before = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) cum[e] = 4 * lane + e < K ? before + c[e] : 0.f;
    const float mk = __shfl(topkp_pick4(cum, (K - 1) & 3), (K - 1) >> 2, 64);   // M_K = C_{|K|-1}
    const float thr = top_p * mk;
    int fail = TABLE_MAX_V;
#pragma unroll
    for (int e = 3; e >= 0; --e) {
        const int p = 4 * lane + e;
        const bool keep = top_p >= 1.f ? ev[e] > 0.f : cum[e] - ev[e] < thr;
        if (p >= 1 && p < K && !keep) fail = p;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) fail = min(fail, __shfl_xor(fail, o, 64));
    n = min(fail, K);
}

// ---- materialise: one wave per listed table row.  PREPASS (the walk's lists): positions < S = |K| only, cum [R, S] f32 and
// tok [R, S] u8; otherwise (the inspection entry point) the whole order as int32 and cum over V columns ------------------------
template <bool PREPASS>
__global__ __launch_bounds__(256) void topkp_rows_kernel(const float* __restrict__ logits, long table_rows,
                                                         const int32_t* __restrict__ rows, long R, int V, float inv_temp, int K,
                                                         float top_p, int32_t* count, void* tokens, float* cum) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= R) return;                                   // wave-uniform
    const long r = rows ? min(max((long)rows[i], 0L), table_rows - 1) : i;
    int tk[4], n;
    float cm[4];
    topkp_row(logits + r * V, V, inv_temp, K, top_p, lane, tk, cm, n);
    const int S = PREPASS ? K : V;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int p = 4 * lane + e;
        if (p < S) {
            if (PREPASS) ((uint8_t*)tokens)[i * S + p] = (uint8_t)tk[e];
            else ((int32_t*)tokens)[i * S + p] = tk[e];
            cum[i * S + p] = cm[e];
        }
    }
    if (lane == 0) count[i] = n;
}

// ---- the walk over the pre-pass lists: one wave per batch row, the seed read from device memory (one captured graph serves
// every seed).  A step issues its row's count and lists together: one dependent round of loads per step.
// MinLenArgs: empty (the top-k / top-p walk) or one WalkMinLen (arcvae_dec_sample_chain_trunc with min_len > 0): the lists a step
// t < min_len reads instead, built with the end token banned ------------------------------------------------------------------
struct WalkMinLen {
    const int32_t* count;
    const float* cum;
    const uint8_t* tok;
    int min_len;
};

template <class... MinLenArgs>
__global__ __launch_bounds__(256) void topkp_walk_kernel(const int32_t* __restrict__ count, const float* __restrict__ cum,
                                                         const uint8_t* __restrict__ tok, int32_t* tokens, int32_t* first_end,
                                                         int B, int V, int S, int max_len, int end_token,
                                                         const unsigned long long* __restrict__ seed_ptr, MinLenArgs... min_len_args) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;                                   // wave-uniform
    const WalkMinLen ml = table_optional<WalkMinLen>(min_len_args...);
    const unsigned long long seed = *seed_ptr;
    const unsigned long long key0 = table_row_key(seed, b);
    int cur = 0, fe = max_len;
    for (int t = 0; t < max_len; ++t) {
        const long r = (long)b * V + cur;
        const bool banned = sizeof...(MinLenArgs) > 0 && t < ml.min_len;          // (false at compile time without the pack)
        const int32_t* __restrict__ count_t = banned ? ml.count : count;
        const float* __restrict__ cum_t = banned ? ml.cum : cum;
        const uint8_t* __restrict__ tok_t = banned ? ml.tok : tok;
        float cm[4];
        int tk[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int p = 4 * lane + e;
            cm[e] = p < S ? cum_t[r * S + p] : 0.f;
            tk[e] = p < S ? (int)tok_t[r * S + p] : 0;
        }
        const int n = min(max(count_t[r], 1), S);
        const float c_last = __shfl(topkp_pick4(cm, (n - 1) & 3), (n - 1) >> 2, 64);
        const unsigned long long rnd = mix64(key0 + (unsigned long long)t);
        const float theta = (float)table_u24(rnd) * (1.0f / 16777216.0f) * c_last;   // 24 uniform bits in [0, 1), times C_{n-1}
        int pick = n - 1;                                 // (no C_i above theta: the last kept position)
#pragma unroll
        for (int e = 3; e >= 0; --e)
            if (4 * lane + e < n && cm[e] > theta) pick = 4 * lane + e;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) pick = min(pick, __shfl_xor(pick, o, 64));
        cur = min(__shfl(topkp_pick4(tk, pick & 3), pick >> 2, 64), V - 1);
        if (lane == 0) tokens[(long)b * max_len + t] = cur;
        if (cur == end_token && fe == max_len) fe = t;
    }
    if (lane == 0) first_end[b] = fe;
}

// ---- min-p, locally typical and banned-token truncation (arcvae_dec_trunc_rows / arcvae_dec_sample_chain_trunc): another way to
// write the same lists.  trunc_row<false> is topkp_row with a banned token (the value part of its key is 0: it sorts behind
// every real token, and |K| <= V - 1 keeps it out) and the min-p test on top of the nucleus test; with min_p = 0 and no ban its
// operations are topkp_row's.  trunc_row<true> re-orders K by d = |log p + H| with a second sort and applies the prefix rule
// in that order ------------------------------------------------------------------------------------------------------------------

// C = the inclusive prefix sums of the wave's 256 masses in position order (in-lane, then across lanes), 0 from position K on:
// the scan of topkp_row, operation for operation
__device__ __forceinline__ void trunc_scan(const float (&ev)[4], int K, int lane, float (&cum)[4]) {
    float c[4], run = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        run += ev[e];
        c[e] = run;
    }
    float incl = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    float before = __shfl_up(incl, 1, 64);
    if (lane == 0) before = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) cum[e] = 4 * lane + e < K ? before + c[e] : 0.f;
}

// n = the first position >= 1 of K that is not kept (|K| if every one is)
__device__ __forceinline__ int trunc_count(const bool (&keep)[4], int K, int lane) {
    int fail = TABLE_MAX_V;
#pragma unroll
    for (int e = 3; e >= 0; --e) {
        const int p = 4 * lane + e;
        if (p >= 1 && p < K && !keep[e]) fail = p;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) fail = min(fail, __shfl_xor(fail, o, 64));
    return min(fail, K);
}

// Outputs as topkp_row; dev = d of each position < |K| and ent = H (wave-uniform) in the typical family, 0 otherwise.
template <bool TYPICAL>
__device__ __forceinline__ void trunc_row(const float* __restrict__ row, int V, float inv_temp, int K, float top_p, float min_p,
                                          float typical_p, int ban, int lane, int (&tok)[4], float (&cum)[4], float (&dev)[4], int& n,
                                          float& ent) {
    unsigned long long key[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int j = 4 * lane + e;
        key[e] = 0ull;
        if (j < V) {
            float s = table_scaled(row[j], inv_temp);
            if (s == 0.f) s = 0.f;                       // -0 folded into +0, as topkp_row
            key[e] = (j == ban ? 0ull : (unsigned long long)ordered_key(s) << 8) | (unsigned long long)(255 - j);
        }
    }
    topkp_sort(key, lane);
    float a[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        tok[e] = 255 - (int)(key[e] & 255ull);
        a[e] = ordered_value((unsigned)(key[e] >> 8));
    }
    const float m = __shfl(a[0], 0, 64);                  // position 0: the row's largest s
    float ev[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        a[e] -= m;                                        // a_i = fl(s_i - s_0)
        ev[e] = 4 * lane + e < K ? expf(a[e]) : 0.f;
    }
    trunc_scan(ev, K, lane, cum);
    const float mk = __shfl(topkp_pick4(cum, (K - 1) & 3), (K - 1) >> 2, 64);   // M_K = C_{|K|-1}
    bool keep[4];
    if (!TYPICAL) {
        const float thr = top_p * mk;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            keep[e] = (top_p >= 1.f ? ev[e] > 0.f : cum[e] - ev[e] < thr) && ev[e] >= min_p;
            dev[e] = 0.f;
        }
        ent = 0.f;
        n = trunc_count(keep, K, lane);
        return;
    }
    // H = -sum e_i * l_i / M_K with l_i = a_i - log M_K (from s, not from e: finite where e_i underflows); lanes in position order
    // in the lane, then one xor butterfly (both partners add the same two numbers: every lane ends with the same bits)
    const float logm = logf(mk);
    float l[4], part = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        l[e] = a[e] - logm;
        if (4 * lane + e < K && ev[e] > 0.f) part += ev[e] * l[e];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    ent = -part / mk;
    // the typical order: d ascending, then the s-position ascending; positions >= |K| keep their place behind K
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int p = 4 * lane + e;
        const unsigned d_bits = __float_as_uint(fabsf(l[e] + ent));
        key[e] = (p < K ? (unsigned long long)(0x7fffffffu - d_bits) << 16 : 0ull) | (unsigned long long)(255 - p) << 8 |
                 (unsigned long long)tok[e];
    }
    topkp_sort(key, lane);
    float em[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int from = 255 - (int)((key[e] >> 8) & 255ull);              // this position's place in the s-order
        tok[e] = (int)(key[e] & 255ull);
        dev[e] = 4 * lane + e < K ? __uint_as_float(0x7fffffffu - (unsigned)(key[e] >> 16)) : 0.f;
        float g[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] = __shfl(ev[i], from >> 2, 64);
        em[e] = topkp_pick4(g, from & 3);                 // e'_q; 0 from |K| on, where nothing moved
    }
    trunc_scan(em, K, lane, cum);
    const float thr = typical_p * __shfl(topkp_pick4(cum, (K - 1) & 3), (K - 1) >> 2, 64);
#pragma unroll
    for (int e = 0; e < 4; ++e) keep[e] = cum[e] - em[e] < thr;
    n = trunc_count(keep, K, lane);
}

// One list set of the rows kernel: where it writes, its |K| and its banned token (-1 = none)
struct TruncSet {
    int32_t* count;
    void* tokens;
    float* cum;
    int K;
    int ban;
};

// As topkp_rows_kernel; S = the lists' row stride (|K| of the plain set in the pre-pass, V otherwise).  blockIdx.y picks the
// list set: 0 the plain one, 1 (the pre-pass of a walk with min_len > 0) the one with the end token banned.
template <bool PREPASS, bool TYPICAL>
__global__ __launch_bounds__(256) void trunc_rows_kernel(const float* __restrict__ logits, long table_rows,
                                                         const int32_t* __restrict__ rows, long R, int V, float inv_temp, int S,
                                                         float top_p, float min_p, float typical_p, TruncSet plain, TruncSet banned,
                                                         float* dev, float* ent) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= R) return;                                   // wave-uniform
    const TruncSet set = blockIdx.y ? banned : plain;
    const long r = rows ? min(max((long)rows[i], 0L), table_rows - 1) : i;
    int tk[4], n;
    float cm[4], dv[4], h;
    trunc_row<TYPICAL>(logits + r * V, V, inv_temp, set.K, top_p, min_p, typical_p, set.ban, lane, tk, cm, dv, n, h);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int p = 4 * lane + e;
        if (p < S) {
            if (PREPASS) ((uint8_t*)set.tokens)[i * S + p] = (uint8_t)tk[e];
            else ((int32_t*)set.tokens)[i * S + p] = tk[e];
            set.cum[i * S + p] = cm[e];
            if (!PREPASS && dev) dev[i * S + p] = dv[e];
        }
    }
    if (lane == 0) {
        set.count[i] = n;
        if (!PREPASS && ent) ent[i] = h;
    }
}

bool topkp_args_ok(int V, float temperature, int top_k, float top_p) {
    return table_vocab_ok(V) && table_temp_ok(temperature, false) && top_k >= 0 && top_p > 0.f && top_p <= 1.f;   // (NaN fails)
}

int topkp_set_size(int V, int top_k) { return top_k == 0 ? V : min(top_k, V); }

// pre-pass lists of B*V rows: count [R] i32 | cum [R, S] f32 | tok [R, S] u8, S = |K|
long topkp_ws_bytes(int B, int V, int top_k) {
    const long R = (long)B * V, S = topkp_set_size(V, top_k);
    return R * 4 + R * S * 4 + R * S;
}

// min_p in [0, 1) (0 = off), typical_p in (0, 1] (1 = off); the typical family takes no nucleus and no min-p.  (A NaN fails.)
bool trunc_args_ok(int V, float temperature, int top_k, float top_p, float min_p, float typical_p) {
    return topkp_args_ok(V, temperature, top_k, top_p) && min_p >= 0.f && min_p < 1.f && typical_p > 0.f && typical_p <= 1.f &&
           (typical_p >= 1.f || (top_p == 1.f && min_p == 0.f));
}

bool trunc_ban_ok(int ban, int V) { return ban == -1 || (ban >= 0 && ban < V && V >= 2); }

// |K| = min(top_k or V, V - 1 with a banned token)
int trunc_set_size(int V, int top_k, int ban) { return min(topkp_set_size(V, top_k), ban >= 0 ? V - 1 : V); }

// one list set, or two with min_len > 0 (the second with the end token banned), each of the top-k / top-p size
long trunc_ws_bytes(int B, int V, int top_k, int min_len) { return (min_len > 0 ? 2 : 1) * topkp_ws_bytes(B, V, top_k); }

// The pre-pass of the list walks (arcvae_dec_sample_chain_trunc, arcvae_dec_sample_draws): lays the list sets out in ws and
// truncates all B*V table rows into them.  set[0]: the plain lists; set[1] (min_len > 0 only, otherwise = set[0]): the lists with
// the end token banned.  The arrays of one kind lie together, count | cum | tok, so that every int32 and fp32 array stays 4-byte
// aligned whatever R * S is
void trunc_prepass(const float* dense_logits, void* ws, int B, int V, int min_len, int end_token, float temperature, int top_k,
                   float top_p, float min_p, float typical_p, hipStream_t stream, TruncSet (&set)[2]) {
    const long R = (long)B * V, S = topkp_set_size(V, top_k), sets = min_len > 0 ? 2 : 1;
    for (long i = 0; i < sets; ++i) {
        int32_t* count = (int32_t*)ws + i * R;
        float* cum = (float*)((int32_t*)ws + sets * R) + i * R * S;
        uint8_t* tok = (uint8_t*)((float*)((int32_t*)ws + sets * R) + sets * R * S) + i * R * S;
        const int ban = i ? end_token : -1;
        set[i] = {count, (void*)tok, cum, trunc_set_size(V, top_k, ban), ban};
    }
    if (sets == 1) set[1] = set[0];
    const dim3 grid((unsigned)((R + 3) / 4), min_len > 0 ? 2 : 1);
    if (typical_p < 1.f)
        hipLaunchKernelGGL((trunc_rows_kernel<true, true>), grid, dim3(256), 0, stream, dense_logits, R, (const int32_t*)nullptr, R,
                           V, 1.0f / temperature, (int)S, top_p, min_p, typical_p, set[0], set[1], (float*)nullptr, (float*)nullptr);
    else
        hipLaunchKernelGGL((trunc_rows_kernel<true, false>), grid, dim3(256), 0, stream, dense_logits, R, (const int32_t*)nullptr, R,
                           V, 1.0f / temperature, (int)S, top_p, min_p, typical_p, set[0], set[1], (float*)nullptr, (float*)nullptr);
}

}  // namespace

extern "C" int arcvae_dec_topkp_rows(const float* dense_logits, long table_rows, const int32_t* rows, long R, int V,
                                     float temperature, int top_k, float top_p, int32_t* count, int32_t* tokens, float* cum,
                                     hipStream_t stream) {
    if (!dense_logits || !count || !tokens || !cum || table_rows <= 0 || R <= 0 || !topkp_args_ok(V, temperature, top_k, top_p))
        return ARCVAE_ERR_ARG;
    if ((!rows && R > table_rows) || (R + 3) / 4 > 0x7fffffffL) return ARCVAE_ERR_ARG;
    hipLaunchKernelGGL(topkp_rows_kernel<false>, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, stream, dense_logits, table_rows, rows,
                       R, V, 1.0f / temperature, topkp_set_size(V, top_k), top_p, count, (void*)tokens, cum);
    return arcvae_launch_status();
}

extern "C" int arcvae_dec_topkp_ws_bytes(int B, int V, int top_k, long* bytes) {
    if (!bytes || B <= 0 || !table_vocab_ok(V) || top_k < 0) return ARCVAE_ERR_ARG;
    *bytes = topkp_ws_bytes(B, V, top_k);
    return ARCVAE_OK;
}

extern "C" int arcvae_dec_sample_chain_topkp(const float* dense_logits, int32_t* tokens, int32_t* first_end, void* ws, long ws_bytes,
                                             int B, int V, int max_len, int end_token, float temperature, int top_k, float top_p,
                                             const unsigned long long* seed, hipStream_t stream) {
    if (!dense_logits || !tokens || !first_end || !ws || !seed || B <= 0 || max_len <= 0 ||
        !topkp_args_ok(V, temperature, top_k, top_p))
        return ARCVAE_ERR_ARG;
    if (ws_bytes < topkp_ws_bytes(B, V, top_k) || ((long)B * V + 3) / 4 > 0x7fffffffL) return ARCVAE_ERR_ARG;
    const long R = (long)B * V, S = topkp_set_size(V, top_k);
    int32_t* count = (int32_t*)ws;
    float* cum = (float*)(count + R);
    uint8_t* tok = (uint8_t*)(cum + R * S);
    hipLaunchKernelGGL(topkp_rows_kernel<true>, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, stream, dense_logits, R,
                       (const int32_t*)nullptr, R, V, 1.0f / temperature, (int)S, top_p, count, (void*)tok, cum);
    hipLaunchKernelGGL(topkp_walk_kernel<>, dim3(ceil_div(B, 4)), dim3(256), 0, stream, count, cum, tok, tokens, first_end, B, V,
                       (int)S, max_len, end_token, seed);
    return arcvae_launch_status();
}

extern "C" int arcvae_dec_trunc_rows(const float* dense_logits, long table_rows, const int32_t* rows, long R, int V,
                                     float temperature, int top_k, float top_p, float min_p, float typical_p, int ban_token,
                                     int32_t* count, int32_t* tokens, float* cum, float* dev, float* ent, hipStream_t stream) {
    if (!dense_logits || !count || !tokens || !cum || table_rows <= 0 || R <= 0 ||
        !trunc_args_ok(V, temperature, top_k, top_p, min_p, typical_p) || !trunc_ban_ok(ban_token, V))
        return ARCVAE_ERR_ARG;
    if ((!rows && R > table_rows) || (R + 3) / 4 > 0x7fffffffL) return ARCVAE_ERR_ARG;
    const TruncSet set = {count, (void*)tokens, cum, trunc_set_size(V, top_k, ban_token), ban_token};
    const dim3 grid((unsigned)((R + 3) / 4));
    if (typical_p < 1.f)
        hipLaunchKernelGGL((trunc_rows_kernel<false, true>), grid, dim3(256), 0, stream, dense_logits, table_rows, rows, R, V,
                           1.0f / temperature, V, top_p, min_p, typical_p, set, set, dev, ent);
    else
        hipLaunchKernelGGL((trunc_rows_kernel<false, false>), grid, dim3(256), 0, stream, dense_logits, table_rows, rows, R, V,
                           1.0f / temperature, V, top_p, min_p, typical_p, set, set, dev, ent);
    return arcvae_launch_status();
}

extern "C" int arcvae_dec_trunc_ws_bytes(int B, int V, int top_k, int min_len, long* bytes) {
    if (!bytes || B <= 0 || !table_vocab_ok(V) || top_k < 0 || min_len < 0) return ARCVAE_ERR_ARG;
    *bytes = trunc_ws_bytes(B, V, top_k, min_len);
    return ARCVAE_OK;
}

extern "C" int arcvae_dec_sample_chain_trunc(const float* dense_logits, int32_t* tokens, int32_t* first_end, void* ws, long ws_bytes,
                                             int B, int V, int max_len, int min_len, int end_token, float temperature, int top_k,
                                             float top_p, float min_p, float typical_p, const unsigned long long* seed,
                                             hipStream_t stream) {
    if (!dense_logits || !tokens || !first_end || !ws || !seed || B <= 0 || max_len <= 0 ||
        !trunc_args_ok(V, temperature, top_k, top_p, min_p, typical_p) || !table_min_len_ok(min_len, max_len) ||
        (min_len > 0 && (!table_end_ok(end_token, V) || V < 2)))
        return ARCVAE_ERR_ARG;
    if (ws_bytes < trunc_ws_bytes(B, V, top_k, min_len) || ((long)B * V + 3) / 4 > 0x7fffffffL) return ARCVAE_ERR_ARG;
    const long S = topkp_set_size(V, top_k);
    TruncSet set[2];
    trunc_prepass(dense_logits, ws, B, V, min_len, end_token, temperature, top_k, top_p, min_p, typical_p, stream, set);
    if (min_len > 0) {
        const WalkMinLen ml = {set[1].count, set[1].cum, (const uint8_t*)set[1].tokens, min_len};
        hipLaunchKernelGGL(topkp_walk_kernel<WalkMinLen>, dim3(ceil_div(B, 4)), dim3(256), 0, stream, set[0].count, set[0].cum,
                           (const uint8_t*)set[0].tokens, tokens, first_end, B, V, (int)S, max_len, end_token, seed, ml);
    } else {
        hipLaunchKernelGGL(topkp_walk_kernel<>, dim3(ceil_div(B, 4)), dim3(256), 0, stream, set[0].count, set[0].cum,
                           (const uint8_t*)set[0].tokens, tokens, first_end, B, V, (int)S, max_len, end_token, seed);
    }
    return arcvae_launch_status();
}

// ---- N independent draws per batch row (arcvae_dec_sample_draws; restated by tests/draws_ref.py): the lists of the pre-pass above,
// walked by ONE THREAD PER DRAW.  A workgroup takes one batch row b and blockDim.x consecutive draws; all its walkers read row b's
// V lists, so it stages them in LDS once (per set: count [V] | cum [V, S] | the token bytes from the dword that holds the first
// one) and a step costs LDS reads only.  STAGED = false is the same body reading the lists where the pre-pass left them (through
// L2): what the launcher takes when the sets exceed the LDS cap -- V = 256 untruncated is 328 KB per set.
// The pick is a front-to-back scan with early exit, four positions a round: C is NOT monotone in fp32 (the pre-pass forms a lane's
// last element as fl(before + run) and the next lane's base in another association order, so C can step down by an ulp at a
// multiple of 4), and the contract's pick is the FIRST position with C_i > theta -- the scan is that rule as written, a bisection
// is not.  In the s-descending family the mass sits at the front: the expected number of reads is the expected rank of the token.
// Workgroup size and LDS cap are read once per process (ARCVAE_DRAWS_WG = 64 | 128 | 256, ARCVAE_DRAWS_LDS_CAP in bytes, 0 = never
// stage) so that tools/bench_draws.py can time the variants.  The defaults are what it measured on the WHOLE call, staging
// included (profiles/draws_bench.json): see there for the figures.
namespace {

struct DrawLists {
    const int32_t* count;
    const float* cum;
    const uint8_t* tok;
};

// key(b, 0) = the row key (draw 0 is the walk above); key(b, d) = mix64(row key ^ (0xD1B54A32D192ED03 * d)), 64-bit wrapping
__device__ __forceinline__ unsigned long long draw_key(unsigned long long row_key, unsigned long long d) {
    return d == 0 ? row_key : mix64(row_key ^ (0xD1B54A32D192ED03ull * d));
}

// dwords of one staged list set: V counts, V*S masses, and the V*S token bytes behind up to 3 bytes of lead (the source is copied
// from the dword that holds its first byte)
__host__ __device__ inline int draws_set_words(int V, int S) { return V + V * S + (V * S + 6) / 4; }

// Copies batch row b's lists (table rows r0 .. r0 + V) of one set into dst; returns the lead: token byte i is byte lead + i of the
// token words.  Whole dwords where the source holds them, single bytes at the tail: nothing is read outside the three arrays.
__device__ __forceinline__ int draws_stage(const DrawLists g, long r0, int V, int S, uint32_t* dst) {
    const int VS = V * S, tid = threadIdx.x, nt = blockDim.x;
    const int32_t* cnt = g.count + r0;
    for (int i = tid; i < V; i += nt) dst[i] = (uint32_t)cnt[i];
    const float* cm = g.cum + r0 * S;
    for (int i = tid; i < VS; i += nt) dst[V + i] = __float_as_uint(cm[i]);
    const uint8_t* tk = g.tok + r0 * S;
    const int lead = (int)((unsigned long long)tk & 3ull);
    const uint8_t* tk_al = tk - lead;                     // (lead > 0: the bytes before tk are the arrays before it in ws)
    const int total = lead + VS, full = total >> 2;
    uint32_t* d32 = dst + V + VS;
    for (int i = tid; i < full; i += nt) d32[i] = ((const uint32_t*)tk_al)[i];
    for (int i = 4 * full + tid; i < total; i += nt) ((uint8_t*)d32)[i] = tk_al[i];
    return lead;
}

// The contract's pick on one list: the first position i < n with C_i > theta, n - 1 if there is none; cum(i) loads C_i (from LDS
// or through L2).  Front to back, four positions a round, out at the first round that holds one.
template <class Load>
__device__ __forceinline__ int draws_pick(int n, float theta, Load cum) {
    for (int i0 = 0; i0 < n; i0 += 4) {
        float c[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) c[e] = i0 + e < n ? cum(i0 + e) : 0.f;
        int hit = -1;
#pragma unroll
        for (int e = 3; e >= 0; --e)
            if (i0 + e < n && c[e] > theta) hit = i0 + e;
        if (hit >= 0) return hit;
    }
    return n - 1;
}

template <bool STAGED, bool MINLEN>
__global__ __launch_bounds__(256) void draws_walk_kernel(DrawLists plain, DrawLists banned, int32_t* __restrict__ tokens,
                                                         int32_t* __restrict__ first_end, int N, int V, int S, int max_len,
                                                         int min_len, int end_token, int pad_token, int chunks,
                                                         const unsigned long long* __restrict__ seed_ptr) {
    extern __shared__ __attribute__((aligned(16))) uint32_t draws_lds[];
    const int b = blockIdx.x / chunks;
    const long d = (long)(blockIdx.x - b * chunks) * blockDim.x + threadIdx.x;
    const long r0 = (long)b * V;
    const int words = draws_set_words(V, S);
    int lead0 = 0, lead1 = 0;
    if (STAGED) {
        lead0 = draws_stage(plain, r0, V, S, draws_lds);
        if (MINLEN) lead1 = draws_stage(banned, r0, V, S, draws_lds + words);
        __syncthreads();
    }
    const bool active = d < N;
    if (!__any(active)) return;                           // wave-uniform (no barrier follows)
    const unsigned long long key0 = draw_key(table_row_key(*seed_ptr, b), (unsigned long long)d);
    int32_t* out = tokens + ((long)b * N + d) * max_len;  // (dereferenced by active threads only)
    const bool pad = pad_token >= 0;
    bool live = active;
    int cur = 0, fe = max_len, t = 0;
    for (; t < max_len; ++t) {
        if (pad && !__any(live)) break;                   // every draw of the wave has ended: the rest is padding
        if (live) {
            const bool ban = MINLEN && t < min_len;
            const unsigned long long rnd = mix64(key0 + (unsigned long long)t);
            int n, pick;
            float theta;
            if (STAGED) {
                const uint32_t* set = draws_lds + (ban ? words : 0);
                const uint32_t* cm = set + V + cur * S;
                n = min(max((int)set[cur], 1), S);
                theta = (float)table_u24(rnd) * (1.0f / 16777216.0f) * __uint_as_float(cm[n - 1]);
                pick = draws_pick(n, theta, [&](int i) { return __uint_as_float(cm[i]); });
                cur = ((const uint8_t*)(set + V + V * S))[(ban ? lead1 : lead0) + cur * S + pick];
            } else {
                const DrawLists g = ban ? banned : plain;
                const long r = r0 + cur;
                const float* __restrict__ cm = g.cum + r * S;
                n = min(max(g.count[r], 1), S);
                theta = (float)table_u24(rnd) * (1.0f / 16777216.0f) * cm[n - 1];
                pick = draws_pick(n, theta, [&](int i) { return cm[i]; });
                cur = g.tok[r * S + pick];
            }
            cur = min(cur, V - 1);
            out[t] = cur;
            if (cur == end_token && fe == max_len) {
                fe = t;
                live = !pad;                              // with a pad token the draw stops consuming steps
            }
        } else if (active) {
            out[t] = pad_token;
        }
    }
    if (active) {
        for (; t < max_len; ++t) out[t] = pad_token;      // (only after the early exit above)
        first_end[(long)b * N + d] = fe;
    }
}

int draws_wg() {
    static const int v = arcvae_env_int("ARCVAE_DRAWS_WG", 128);
    return v == 256 ? 256 : (v == 64 ? 64 : 128);
}

// the largest staged image, both sets together: 64 KB is what a workgroup gets without asking the runtime for more, and two
// sets of the V = S = 80 workload (64 648 bytes) still fit
long draws_lds_cap() {
    static const int v = arcvae_env_int("ARCVAE_DRAWS_LDS_CAP", 64 * 1024);
    return v < 0 ? 0 : (v > 64 * 1024 ? 64 * 1024 : v);
}

template <bool STAGED, bool MINLEN>
void draws_launch(unsigned blocks, int wg, size_t lds, const DrawLists& plain, const DrawLists& banned, int32_t* tokens,
                  int32_t* first_end, int N, int V, int S, int max_len, int min_len, int end_token, int pad_token, int chunks,
                  const unsigned long long* seed, hipStream_t stream) {
    hipLaunchKernelGGL((draws_walk_kernel<STAGED, MINLEN>), dim3(blocks), dim3(wg), lds, stream, plain, banned, tokens, first_end, N,
                       V, S, max_len, min_len, end_token, pad_token, chunks, seed);
}

}  // namespace

extern "C" int arcvae_dec_sample_draws_ws_bytes(int B, int V, int top_k, int min_len, long* bytes) {
    return arcvae_dec_trunc_ws_bytes(B, V, top_k, min_len, bytes);
}

extern "C" int arcvae_dec_sample_draws(const float* dense_logits, int32_t* tokens, int32_t* first_end, void* ws, long ws_bytes, int B,
                                       int N, int V, int max_len, int min_len, int end_token, int pad_token, float temperature,
                                       int top_k, float top_p, float min_p, float typical_p, const unsigned long long* seed,
                                       hipStream_t stream) {
    if (!dense_logits || !tokens || !first_end || !ws || !seed || B <= 0 || N <= 0 || max_len <= 0 ||
        !trunc_args_ok(V, temperature, top_k, top_p, min_p, typical_p) || !table_min_len_ok(min_len, max_len) ||
        (min_len > 0 && (!table_end_ok(end_token, V) || V < 2)) || !(pad_token == -1 || table_pad_ok(pad_token)))
        return ARCVAE_ERR_ARG;
    if (ws_bytes < trunc_ws_bytes(B, V, top_k, min_len) || ((long)B * V + 3) / 4 > 0x7fffffffL) return ARCVAE_ERR_ARG;
    if ((long)B * N > 0x7fffffffL || (long)B * N * max_len > (1L << 60)) return ARCVAE_ERR_ARG;   // draw and output indices
    if ((long)B * ((long)N + 255) > 0xffffffffL) return ARCVAE_ERR_ARG;       // the launch: B * ceil(N / w) workgroups of w <= 256 threads
    const int S = topkp_set_size(V, top_k);
    TruncSet set[2];
    trunc_prepass(dense_logits, ws, B, V, min_len, end_token, temperature, top_k, top_p, min_p, typical_p, stream, set);
    const DrawLists plain = {set[0].count, set[0].cum, (const uint8_t*)set[0].tokens};
    const DrawLists banned = {set[1].count, set[1].cum, (const uint8_t*)set[1].tokens};
    const int wg = draws_wg(), chunks = (int)(((long)N + wg - 1) / wg);
    const unsigned blocks = (unsigned)((long)B * chunks);
    const long lds = (long)(min_len > 0 ? 2 : 1) * draws_set_words(V, S) * 4;
    const bool staged = lds <= draws_lds_cap();
#define DRAWS_LAUNCH(ST, ML)                                                                                                     \
    draws_launch<ST, ML>(blocks, wg, ST ? (size_t)lds : 0, plain, banned, tokens, first_end, N, V, S, max_len, min_len, end_token, \
                         pad_token, chunks, seed, stream)
    if (staged && min_len > 0) DRAWS_LAUNCH(true, true);
    else if (staged) DRAWS_LAUNCH(true, false);
    else if (min_len > 0) DRAWS_LAUNCH(false, true);
    else DRAWS_LAUNCH(false, false);
#undef DRAWS_LAUNCH
    return arcvae_launch_status();
}
