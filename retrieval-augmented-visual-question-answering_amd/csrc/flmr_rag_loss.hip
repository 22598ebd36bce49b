// Token log-likelihoods of the RAG-sequence marginalised loss and their backward (RagModelForBlip.get_loss,
// src/models/rag/rag_model_blip.py:859-890: log_softmax(seq_logits).gather(-1, target), masked): flmr_rag_token_ll_fwd / _bwd.
//
// Both kernels stream the [R, T, V] logits once, one workgroup of 4 waves per token row (r, t), 16 bytes per lane per load, four
// loads in flight per lane.  A row whose target is ignore_index is not read: the forward writes ll = 0 and lse = (0, 0) for it, the backward
// writes its V zeros.  The logits are fp32, fp16 or bf16 and are widened exactly; every sum is fp32.
//   forward:  every lane keeps an online (max, sum) pair over its share of the row (the maximum starts at -inf; a vector's sum is
//             rescaled only when the vector raises the maximum); the pairs are merged by a butterfly over the wave, then by lane 0
//             of wave 0 over the four waves in ascending order: a fixed tree, so two calls give the same bits.
//             lse is kept as its two words (max, log(sum)) and ll = (x[target] - max) - log(sum): x - max is exact or nearly so
//             and log(sum) is small wherever a probability is large, so exp((x - max) - log(sum)) near 1 keeps an absolute error of
//             ~6e-8, where exp(x - fl(max + log(sum))) carries the rounding of a number of magnitude ~10 (~5e-7) into 1 - p.
//             Row (r, 0) also tracks (value, lowest index) of its maximum.
//   backward: dlogits[v] = g * ([v == target] - exp((x[v] - max) - log(sum))), rounded once to the logits' dtype.
// Rows need not be 16-byte aligned (odd V with a 2-byte type, a [..., :V] view).  The forward counts its 16-byte vectors from the
// row's first element and reads a row that does not start on a 16-byte boundary with element-aligned loads (the compiler picks
// the instructions that alignment allows), so the lane that takes an element, and every bit of lse, is the same for a view and
// for its contiguous copy.  The backward is elementwise: it walks the row it WRITES as a scalar head up to the first 16-byte
// boundary, an aligned vector body and a scalar tail, and reads with element-aligned loads where the input row sits at another
// offset inside its 16 bytes.
// exp is v_exp_f32 on an argument whose product with log2(e) carries its rounding error along (rag_exp): ~1 ulp, as libm's.
#include "flmr_device.h"

#define RL_THREADS 256
#define RL_WAVES (RL_THREADS / FLMR_WAVE)
#define RL_DEPTH 4   // 16-byte loads in flight per lane

typedef uint32_t rl_u4 __attribute__((ext_vector_type(4)));
struct rl_bf16 { uint16_t bits; };

template <typename T> struct rl_traits { static constexpr int EPV = 16 / (int)sizeof(T); };

__device__ __forceinline__ float rl_widen(float v) { return v; }
__device__ __forceinline__ float rl_widen(_Float16 v) { return (float)v; }
__device__ __forceinline__ float rl_widen(rl_bf16 v) { return __uint_as_float((uint32_t)v.bits << 16); }

__device__ __forceinline__ void rl_narrow(float v, float& o) { o = v; }
__device__ __forceinline__ void rl_narrow(float v, _Float16& o) { o = (_Float16)v; }   // round to nearest-even
__device__ __forceinline__ void rl_narrow(float v, rl_bf16& o) {
    const uint32_t u = __float_as_uint(v);
    o.bits = (v != v) ? (uint16_t)0x7fc0 : (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);   // round to nearest-even
}

template <typename T> struct alignas(16) rl_vec { T e[rl_traits<T>::EPV]; };

// 16 bytes at p: ALIGNED -> one 16-byte load (p is a multiple of 16); else p is only element-aligned
template <typename T, bool ALIGNED>
__device__ __forceinline__ rl_vec<T> rl_load(const T* p) {
    rl_vec<T> v;
    if constexpr (ALIGNED) {
        *reinterpret_cast<rl_u4*>(&v) = *reinterpret_cast<const rl_u4*>(p);
    } else {
        __builtin_memcpy(&v, p, 16);
    }
    return v;
}

// exp(d) for d <= 0 or barely above (d = -inf included): 2^(d * log2 e) with the product's rounding error and log2 e's low part applied to first order
__device__ __forceinline__ float rag_exp(float d) {
    const float L2E_HI = 1.44269502162933349609375f, L2E_LO = 1.92596299112661746e-8f, LN2 = 0.693147182464599609375f;
    d = fmaxf(d, -200.0f);                                   // exp(-200) = 0 in fp32; keeps -inf out of the error term
    const float t = d * L2E_HI;
    const float lo = fmaf(d, L2E_HI, -t) + d * L2E_LO;
    const float e = __builtin_amdgcn_exp2f(t);
    return fmaf(e, lo * LN2, e);
}

struct rl_ms { float m, s; };   // sum of exp(x - m) over the elements seen; m = -inf, s = 0: none yet
__device__ __forceinline__ rl_ms rl_merge(rl_ms a, rl_ms b) {
    const float m = fmaxf(a.m, b.m);
    if (m == FLMR_NEG_INF) return rl_ms{m, 0.0f};
    return rl_ms{m, a.s * rag_exp(a.m - m) + b.s * rag_exp(b.m - m)};
}
struct rl_best { float v; int i; };   // the maximum and its lowest index (i = INT_MAX: none yet)
__device__ __forceinline__ rl_best rl_better(rl_best a, rl_best b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }

template <bool ARG>
__device__ __forceinline__ void rl_take(const float* x, int n, int64_t i0, rl_ms& acc, rl_best& best) {
    float vmax = x[0];
    for (int k = 1; k < n; k++) vmax = fmaxf(vmax, x[k]);
    if (vmax > acc.m) {
        acc.s *= rag_exp(acc.m - vmax);   // (acc.m = -inf: s is 0 and stays 0)
        acc.m = vmax;
    }
    if (acc.m != FLMR_NEG_INF) {
        float s = 0.0f;
        for (int k = 0; k < n; k++) s += rag_exp(x[k] - acc.m);
        acc.s += s;
    }
    if constexpr (ARG) {
        for (int k = 0; k < n; k++) best = rl_better(best, rl_best{x[k], (int)(i0 + k)});
    }
}

// the row split at the 16-byte boundaries of `anchor` (the pointer whose accesses are the vector ones)
template <typename T>
__device__ __forceinline__ void rl_split(const T* anchor, int64_t V, int& head, int64_t& nvec) {
    constexpr int EPV = rl_traits<T>::EPV;
    const int mis = (int)((reinterpret_cast<uintptr_t>(anchor) & 15) / sizeof(T));
    const int64_t h = mis ? EPV - mis : 0;
    head = (int)(h < V ? h : V);
    nvec = (V - head) / EPV;
}

template <typename T, bool ARG, bool ALIGNED>
__device__ __forceinline__ void rl_fwd_row(const T* __restrict__ x, int64_t V, int64_t tgt, bool live, float* ll, float2* lse,
                                           int32_t* first_argmax, rl_ms* s_ms, rl_best* s_best) {
    constexpr int EPV = rl_traits<T>::EPV;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // vectors are counted from the row's first element, wherever it lies: which lane takes which element -- and with it every
    // bit of the result -- does not depend on the row's address (a view and its contiguous copy agree exactly)
    const int64_t nvec = V / EPV, tail0 = nvec * EPV;
    rl_ms acc{FLMR_NEG_INF, 0.0f};
    rl_best best{FLMR_NEG_INF, 0x7fffffff};
    if (tid < V - tail0) {   // the scalar tail: at most EPV - 1 elements, one per lane of wave 0
        const float v = rl_widen(x[tail0 + tid]);
        rl_take<ARG>(&v, 1, tail0 + tid, acc, best);
    }
    for (int64_t base = 0; base < nvec; base += (int64_t)RL_THREADS * RL_DEPTH) {
        rl_vec<T> raw[RL_DEPTH];
#pragma unroll
        for (int k = 0; k < RL_DEPTH; k++) {
            const int64_t iv = base + (int64_t)k * RL_THREADS + tid;
            if (iv < nvec) raw[k] = rl_load<T, ALIGNED>(x + iv * EPV);
        }
#pragma unroll
        for (int k = 0; k < RL_DEPTH; k++) {
            const int64_t iv = base + (int64_t)k * RL_THREADS + tid;
            if (iv < nvec) {
                float f[EPV];
#pragma unroll
                for (int e = 0; e < EPV; e++) f[e] = rl_widen(raw[k].e[e]);
                rl_take<ARG>(f, EPV, iv * EPV, acc, best);
            }
        }
    }
    // lanes: butterfly, lane 0's tree is the result; waves: ascending, by one lane
    for (int off = 32; off >= 1; off >>= 1) {
        acc = rl_merge(acc, rl_ms{__shfl_xor(acc.m, off, 64), __shfl_xor(acc.s, off, 64)});
        if constexpr (ARG) best = rl_better(best, rl_best{__shfl_xor(best.v, off, 64), __shfl_xor(best.i, off, 64)});
    }
    if (lane == 0) {
        s_ms[wave] = acc;
        if constexpr (ARG) s_best[wave] = best;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < RL_WAVES; w++) {
            acc = rl_merge(acc, s_ms[w]);
            if constexpr (ARG) best = rl_better(best, s_best[w]);
        }
        if constexpr (ARG) {
            if (first_argmax) *first_argmax = best.i == 0x7fffffff ? 0 : best.i;   // (a row of NaNs: no comparison holds)
        }
        if (live) {
            const float logs = logf(acc.s);
            *lse = make_float2(acc.m, logs);
            *ll = (rl_widen(x[tgt]) - acc.m) - logs;
        } else {
            *lse = make_float2(0.0f, 0.0f);
            *ll = 0.0f;
        }
    }
    __syncthreads();   // (s_ms is reused by the workgroup's next row)
}

template <typename T>
__global__ __launch_bounds__(RL_THREADS) void rag_token_ll_fwd_kernel(const T* __restrict__ logits, int64_t rows, int64_t T_, int64_t V,
                                                                      int64_t stride_r, int64_t stride_t,
                                                                      const int64_t* __restrict__ target, int64_t ignore_index,
                                                                      float* __restrict__ ll, float2* __restrict__ lse,
                                                                      int32_t* __restrict__ first_argmax) {
    __shared__ rl_ms s_ms[RL_WAVES];
    __shared__ rl_best s_best[RL_WAVES];
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int64_t r = row / T_, t = row - r * T_;
        const int64_t tgt = target[row];
        const bool live = tgt != ignore_index && tgt >= 0 && tgt < V;
        const T* x = logits + r * stride_r + t * stride_t;
        const bool aligned = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
        if (t == 0) {
            int32_t* fa = first_argmax ? first_argmax + r : nullptr;
            if (aligned) rl_fwd_row<T, true, true>(x, V, tgt, live, ll + row, lse + row, fa, s_ms, s_best);
            else rl_fwd_row<T, true, false>(x, V, tgt, live, ll + row, lse + row, fa, s_ms, s_best);
        } else if (live) {
            if (aligned) rl_fwd_row<T, false, true>(x, V, tgt, live, ll + row, lse + row, nullptr, s_ms, s_best);
            else rl_fwd_row<T, false, false>(x, V, tgt, live, ll + row, lse + row, nullptr, s_ms, s_best);
        } else if (threadIdx.x == 0) {
            ll[row] = 0.0f;
            lse[row] = make_float2(0.0f, 0.0f);
        }
    }
}

template <typename T, bool ALIGNED>
__device__ __forceinline__ void rl_bwd_body(const T* __restrict__ x, T* __restrict__ out, int head, int64_t nvec, int64_t tgt, float g,
                                            float2 lse) {
    constexpr int EPV = rl_traits<T>::EPV;
    const int tid = threadIdx.x;
    for (int64_t base = 0; base < nvec; base += (int64_t)RL_THREADS * RL_DEPTH) {
        rl_vec<T> raw[RL_DEPTH];
#pragma unroll
        for (int k = 0; k < RL_DEPTH; k++) {
            const int64_t iv = base + (int64_t)k * RL_THREADS + tid;
            if (iv < nvec) raw[k] = rl_load<T, ALIGNED>(x + head + iv * EPV);
        }
#pragma unroll
        for (int k = 0; k < RL_DEPTH; k++) {
            const int64_t iv = base + (int64_t)k * RL_THREADS + tid;
            if (iv < nvec) {
                const int64_t i0 = head + iv * EPV;
                rl_vec<T> o;
#pragma unroll
                for (int e = 0; e < EPV; e++) {
                    const float p = rag_exp((rl_widen(raw[k].e[e]) - lse.x) - lse.y);
                    rl_narrow(g * ((i0 + e == tgt ? 1.0f : 0.0f) - p), o.e[e]);
                }
                *reinterpret_cast<rl_u4*>(out + i0) = *reinterpret_cast<const rl_u4*>(&o);
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(RL_THREADS) void rag_token_ll_bwd_kernel(const T* __restrict__ logits, int64_t rows, int64_t T_, int64_t V,
                                                                      int64_t stride_r, int64_t stride_t,
                                                                      const int64_t* __restrict__ target, int64_t ignore_index,
                                                                      const float2* __restrict__ lse, const float* __restrict__ grad_ll,
                                                                      T* __restrict__ dlogits) {
    constexpr int EPV = rl_traits<T>::EPV;
    const int tid = threadIdx.x;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int64_t r = row / T_, t = row - r * T_;
        const int64_t tgt = target[row];
        const bool live = tgt != ignore_index && tgt >= 0 && tgt < V;
        T* out = dlogits + row * V;
        int head;
        int64_t nvec;
        rl_split(out, V, head, nvec);
        const int64_t tail0 = head + nvec * EPV;
        if (!live) {
            T zero;
            rl_narrow(0.0f, zero);
            if (tid < head) out[tid] = zero;
            if (tid < V - tail0) out[tail0 + tid] = zero;
            const rl_u4 z = {0u, 0u, 0u, 0u};
            for (int64_t iv = tid; iv < nvec; iv += RL_THREADS) *reinterpret_cast<rl_u4*>(out + head + iv * EPV) = z;
            continue;
        }
        const T* x = logits + r * stride_r + t * stride_t;
        const float g = grad_ll[row];
        const float2 l = lse[row];
        if (tid < head) {
            const float p = rag_exp((rl_widen(x[tid]) - l.x) - l.y);
            rl_narrow(g * ((tid == tgt ? 1.0f : 0.0f) - p), out[tid]);
        }
        if (tid < V - tail0) {
            const int64_t i = tail0 + tid;
            const float p = rag_exp((rl_widen(x[i]) - l.x) - l.y);
            rl_narrow(g * ((i == tgt ? 1.0f : 0.0f) - p), out[i]);
        }
        if ((reinterpret_cast<uintptr_t>(x + head) & 15) == 0) {
            rl_bwd_body<T, true>(x, out, head, nvec, tgt, g, l);
        } else {
            rl_bwd_body<T, false>(x, out, head, nvec, tgt, g, l);
        }
    }
}

static int rl_check(const void* logits, int32_t dtype, int64_t R, int64_t T, int64_t V, int64_t stride_r, int64_t stride_t,
                    const void* target, int64_t* rows, unsigned* grid) {
    if (dtype != FLMR_F32 && dtype != FLMR_F16 && dtype != FLMR_BF16)
        FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "dtype=%d (FLMR_F32, FLMR_F16 or FLMR_BF16)", dtype);
    if (stride_r < 0 || stride_t < 0) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "negative strides (%lld, %lld)", (long long)stride_r, (long long)stride_t);
    if (R < 0 || T < 0 || V < 1) FLMR_FAIL(FLMR_ERR_INVALID, "bad sizes R=%lld T=%lld V=%lld", (long long)R, (long long)T, (long long)V);
    *rows = R * T;
    if (*rows == 0) return FLMR_OK;
    if (!logits || !target) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    if (reinterpret_cast<uintptr_t>(logits) & (dtype == FLMR_F32 ? 3 : 1)) FLMR_FAIL(FLMR_ERR_INVALID, "logits not aligned to their element");
    if (reinterpret_cast<uintptr_t>(target) & 7) FLMR_FAIL(FLMR_ERR_INVALID, "target not aligned to 8 bytes");
    *grid = (unsigned)(*rows < (1 << 20) ? *rows : (1 << 20));   // one workgroup per token row; beyond 2^20 rows they stride
    return FLMR_OK;
}

extern "C" int flmr_rag_token_ll_fwd(const void* logits, int32_t dtype, int64_t R, int64_t T, int64_t V, int64_t stride_r, int64_t stride_t,
                                     const int64_t* target, int64_t ignore_index, float* ll, float* lse, int32_t* first_argmax,
                                     flmr_stream_t stream) {
    int64_t rows = 0;
    unsigned grid = 0;
    const int rc = rl_check(logits, dtype, R, T, V, stride_r, stride_t, target, &rows, &grid);
    if (rc || rows == 0) return rc;
    if (!ll || !lse) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    if (reinterpret_cast<uintptr_t>(lse) & 7) FLMR_FAIL(FLMR_ERR_INVALID, "lse not aligned to 8 bytes");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define RL_FWD(TY)                                                                                                                  \
    hipLaunchKernelGGL((rag_token_ll_fwd_kernel<TY>), dim3(grid), dim3(RL_THREADS), 0, st, static_cast<const TY*>(logits), rows, T, V, \
                       stride_r, stride_t, target, ignore_index, ll, reinterpret_cast<float2*>(lse), first_argmax)
    if (dtype == FLMR_F32) RL_FWD(float);
    else if (dtype == FLMR_F16) RL_FWD(_Float16);
    else RL_FWD(rl_bf16);
#undef RL_FWD
    FLMR_LAUNCH_CHECK();
    return FLMR_OK;
}

extern "C" int flmr_rag_token_ll_bwd(const void* logits, int32_t dtype, int64_t R, int64_t T, int64_t V, int64_t stride_r, int64_t stride_t,
                                     const int64_t* target, int64_t ignore_index, const float* lse, const float* grad_ll, void* dlogits,
                                     flmr_stream_t stream) {
    int64_t rows = 0;
    unsigned grid = 0;
    const int rc = rl_check(logits, dtype, R, T, V, stride_r, stride_t, target, &rows, &grid);
    if (rc || rows == 0) return rc;
    if (!lse || !grad_ll || !dlogits) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    if (reinterpret_cast<uintptr_t>(lse) & 7) FLMR_FAIL(FLMR_ERR_INVALID, "lse not aligned to 8 bytes");
    if (reinterpret_cast<uintptr_t>(dlogits) & (dtype == FLMR_F32 ? 3 : 1)) FLMR_FAIL(FLMR_ERR_INVALID, "dlogits not aligned to their element");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define RL_BWD(TY)                                                                                                                  \
    hipLaunchKernelGGL((rag_token_ll_bwd_kernel<TY>), dim3(grid), dim3(RL_THREADS), 0, st, static_cast<const TY*>(logits), rows, T, V, \
                       stride_r, stride_t, target, ignore_index, reinterpret_cast<const float2*>(lse), grad_ll, static_cast<TY*>(dlogits))
    if (dtype == FLMR_F32) RL_BWD(float);
    else if (dtype == FLMR_F16) RL_BWD(_Float16);
    else RL_BWD(rl_bf16);
#undef RL_BWD
    FLMR_LAUNCH_CHECK();
    return FLMR_OK;
}
