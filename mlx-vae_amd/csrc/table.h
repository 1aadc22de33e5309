// What the decoders of the dense table [B*V, V] share (beam, chain, kbest, sample, swor, table .hip): the contract is the block
// "dense-table decoders: common contract" of include/arcvae_hip.h.  Included by those six files only: decoder.hip's categorical
// walk keeps its own copy of the row generator, so that no file of the training step depends on this header.
#pragma once
#include "common.h"

constexpr int TABLE_MAX_V = 256;             // a token, a parent token and a pad token fit in one byte
constexpr int TABLE_MAX_K = 32;              // widest beam / list / sample per batch row

// The step term lp(c, v) = fl(fl(x[b*V+c, v] * inv_temp) - lse[b*V+c]): one multiplication and one subtraction, each rounded
// once.  Every bit-for-bit promise of these decoders (against each other, arcvae_dec_sequence_logprob and the fp32 restatements
// in tests/) rests on this order, and on -ffp-contract=off: fused into fma(x, inv_temp, -l) the product is not rounded.
__device__ __forceinline__ float table_scaled(float x, float inv_temp) { return x * inv_temp; }
__device__ __forceinline__ float table_lp(float x, float l, float inv_temp) { return table_scaled(x, inv_temp) - l; }

// Order-preserving integer image of a float: a > b (neither a NaN) <=> ordered_key(a) > ordered_key(b).  -0 and +0 compare
// equal and have different keys: a caller whose tie order must not see the sign folds -0 into +0 first.
__device__ __forceinline__ unsigned ordered_key(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ordered_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(v, o, 64);
        v = other > v ? other : v;
    }
    return v;
}

// The counter-based generator of the sampling decoders: a batch row's key, and the 24 uniform bits of a draw (its top ones).
__device__ __forceinline__ unsigned long long table_row_key(unsigned long long seed, int b) {
    return mix64(seed ^ ((unsigned long long)b << 32));
}
__device__ __forceinline__ unsigned table_u24(unsigned long long h) { return (unsigned)(h >> 40); }

// Back pointers of the K-slot walks, uint16 [B, max_len, K]: parent slot | token << 8.
__device__ __forceinline__ uint16_t table_bp_pack(int parent, int tok) { return (uint16_t)((parent & 255) | ((tok & 255) << 8)); }

// Slot `slot` of batch row b after t_end steps, followed back into out [max_len]; pad_token from t_end on, and everywhere when
// the slot is not `filled`.  Returns the length: 0 for an empty slot, else the first end_token's index + 1 (max_len without one).
__device__ __forceinline__ int table_backtrack(const uint16_t* bp, int32_t* out, int b, int slot, int K, int t_end, int max_len,
                                               int end_token, int pad_token, bool filled) {
    for (int t = t_end; t < max_len; ++t) out[t] = pad_token;
    if (!filled) {
        for (int t = 0; t < t_end; ++t) out[t] = pad_token;
        return 0;
    }
    int fe = max_len;
    for (int t = t_end - 1; t >= 0; --t) {
        const uint16_t v = bp[((long)b * max_len + t) * K + slot];
        const int tok = v >> 8;
        out[t] = tok;
        if (tok == end_token) fe = t;
        slot = min((int)(v & 255), K - 1);               // (clamped: a row outside the contract stays inside the slots)
    }
    return fe < max_len ? fe + 1 : max_len;
}

// A kernel with optional extra arguments takes them as a pack that is empty or one struct T: the struct, all zero for no pack.
template <class T, class... Args>
__device__ __forceinline__ T table_optional(Args... a) { return T{a...}; }

// ---- host: the argument checks the entry points share.  An entry point that has no K (or no V) passes 1 ---------------------
static inline bool table_vocab_ok(int V) { return V >= 1 && V <= TABLE_MAX_V; }
static inline bool table_dims_ok(int B, int V, int K, int max_len) {
    return B > 0 && table_vocab_ok(V) && K >= 1 && K <= TABLE_MAX_K && max_len >= 1;
}
// finite: chain.hip, kbest.hip and the row costs refuse +inf; beam, swor, top-k/p and the table's own functions take it (inv_temp = 0: every
// row uniform).  A NaN fails either way.
static inline bool table_temp_ok(float temperature, bool finite) {
    return temperature > 0.f && (!finite || temperature <= 3.402823466e+38f);
}
static inline bool table_pad_ok(int pad_token) { return pad_token >= 0 && pad_token <= 255; }   // back pointers keep 8 bits
static inline bool table_min_len_ok(int min_len, int max_len) { return min_len >= 0 && min_len <= max_len; }
// chain.hip and kbest.hip index by end_token; beam, swor, top-k/p and sequence_logprob only compare it and take any value.
static inline bool table_end_ok(int end_token, int V) { return end_token >= 0 && end_token < V; }
