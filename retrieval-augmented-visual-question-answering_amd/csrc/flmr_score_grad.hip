// Backward of the padded MaxSim (TPC/modeling/colbert.py:235-286 under autograd): flmr_colbert_maxsim_bwd.
//
// The forward (flmr_colbert_maxsim_fwd, flmr_ops.hip) records the winning token j*(r, i) of every output row r and query
// column i (-1: no gradient).  With G = dL/dcolmax:
//   dQ[qr, i, :] = sum over the rows r of query row qr, in ascending document order, of G[r, i] * D[doc(r), j*(r, i), :]
//   dD[b, j, :]  = sum over the entries (q, i) of document b whose winner is j, in ascending (q, i) order, of G[r, i] * Q[q, i, :]
// Both are gathers in a fixed order: no floating-point atomics, so two calls give bit-identical gradients.  The sums are fp32
// throughout.  The operand read (D for dQ, Q for dD) and the gradient written are each fp32 or fp16 (flmr_colbert_maxsim_bwd_typed):
// an fp16 operand is read as half2 and widened exactly, an fp16 gradient is the fp32 sum rounded once to nearest-even on the
// store -- the bits of the fp32 gradient of the widened operands converted to half.  The fp32 instantiations are the kernels as
// they were.
#include "flmr_device.h"

#define SG_TILE 64   // document tokens per dD workgroup (16 per wave)

typedef _Float16 sgh2 __attribute__((ext_vector_type(2)));
template <typename T>
__device__ __forceinline__ float2 sg_load2(const T* p) {
    if constexpr (sizeof(T) == 2) {
        const sgh2 v = *reinterpret_cast<const sgh2*>(p);
        return make_float2((float)v[0], (float)v[1]);
    } else {
        return *reinterpret_cast<const float2*>(p);
    }
}
template <typename T>
__device__ __forceinline__ void sg_store2(T* p, float2 v) {
    if constexpr (sizeof(T) == 2) {
        sgh2 o;
        o[0] = (_Float16)v.x;   // round to nearest-even
        o[1] = (_Float16)v.y;
        *reinterpret_cast<sgh2*>(p) = o;
    } else {
        *reinterpret_cast<float2*>(p) = v;
    }
}

// one wave per (query row qr, column i); lane l owns dims 2l, 2l+1
template <typename TD, typename TO>
__global__ __launch_bounds__(256) void maxsim_grad_q_kernel(const TD* __restrict__ D, const int32_t* __restrict__ argmax,
                                                            const float* __restrict__ G, int q_rows, int nq, int B, int Ld,
                                                            int cross, int q_batch, TO* __restrict__ dQ) {
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= (int64_t)q_rows * nq) return;
    const int qr = (int)(pair / nq), i = (int)(pair % nq);
    // the output rows that read query row qr: every document (cross, or the broadcast q_batch == 1), else row qr alone
    const int nb = (cross || q_batch == 1) ? B : 1;
    float2 acc = make_float2(0.0f, 0.0f);
    for (int k0 = 0; k0 < nb; k0 += 64) {
        const int kk = k0 + lane;
        int a_l = -1;
        float g_l = 0.0f;
        if (kk < nb) {
            const int b = nb == 1 ? qr : kk;
            const size_t r = cross ? (size_t)qr * B + b : (size_t)b;
            a_l = argmax[r * nq + i];
            g_l = G[r * nq + i];
        }
        const int n = nb - k0 < 64 ? nb - k0 : 64;
        for (int j = 0; j < n; j++) {
            const int a = __shfl(a_l, j, 64);
            const float g = __shfl(g_l, j, 64);
            if (a < 0) continue;
            const int b = nb == 1 ? qr : k0 + j;
            const float2 d = sg_load2(D + ((size_t)b * Ld + a) * FLMR_DIM + 2 * lane);
            acc.x = fmaf(g, d.x, acc.x);
            acc.y = fmaf(g, d.y, acc.y);
        }
    }
    sg_store2(dQ + (size_t)pair * FLMR_DIM + 2 * lane, acc);
}

// one workgroup per (token tile, document b); wave w owns tokens tile*64 + 16w .. +15 and accumulates them in LDS, lane l
// dims 2l, 2l+1.  Every wave walks all (q, i) entries of its document 64 at a time; a ballot picks the entries whose winner
// is one of its tokens and they are added in ascending order.  Each LDS slot is touched by one lane only.
template <typename TQ, typename TO>
__global__ __launch_bounds__(256) void maxsim_grad_d_kernel(const TQ* __restrict__ Q, const int32_t* __restrict__ argmax,
                                                            const float* __restrict__ G, int nq, int B, int Ld, int cross,
                                                            int q_batch, TO* __restrict__ dD) {
    __shared__ __attribute__((aligned(16))) float2 acc[SG_TILE][FLMR_DIM / 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * SG_TILE + wave * 16;
    for (int t = 0; t < 16; t++) acc[wave * 16 + t][lane] = make_float2(0.0f, 0.0f);
    const int nrq = cross ? q_batch : 1;        // output rows per document
    const int64_t E = (int64_t)nrq * nq;
    for (int64_t e0 = 0; e0 < E; e0 += 64) {
        const int64_t e = e0 + lane;
        int a_l = -1;
        float g_l = 0.0f;
        if (e < E) {
            const int q = (int)(e / nq), i = (int)(e % nq);
            const size_t r = cross ? (size_t)q * B + b : (size_t)b;
            a_l = argmax[r * nq + i];
            if (a_l >= t0 && a_l < t0 + 16) g_l = G[r * nq + i];
        }
        uint64_t hits = __ballot(a_l >= t0 && a_l < t0 + 16);
        while (hits) {
            const int l = __ffsll((unsigned long long)hits) - 1;
            hits &= hits - 1;
            const int tok = __shfl(a_l, l, 64);
            const float g = __shfl(g_l, l, 64);
            const int64_t ee = e0 + l;
            const int q = (int)(ee / nq), i = (int)(ee % nq);
            const int qs = cross ? q : (q_batch == 1 ? 0 : b);
            const float2 qv = sg_load2(Q + ((size_t)qs * nq + i) * FLMR_DIM + 2 * lane);
            float2& s = acc[tok - t0 + wave * 16][lane];
            s.x = fmaf(g, qv.x, s.x);
            s.y = fmaf(g, qv.y, s.y);
        }
    }
    for (int t = 0; t < 16; t++) {
        const int tok = t0 + t;
        if (tok < Ld) sg_store2(dD + ((size_t)b * Ld + tok) * FLMR_DIM + 2 * lane, acc[wave * 16 + t][lane]);
    }
}

template <typename TD, typename TO>
static int launch_grad_q(const void* D, const int32_t* argmax, const float* G, int32_t q_batch, int32_t nq, int32_t B, int32_t Ld,
                         int32_t cross, void* dQ, hipStream_t st) {
    const int64_t pairs = (int64_t)q_batch * nq;
    hipLaunchKernelGGL((maxsim_grad_q_kernel<TD, TO>), dim3((unsigned)flmr_ceil_div(pairs, 4)), dim3(256), 0, st,
                       static_cast<const TD*>(D), argmax, G, (int)q_batch, (int)nq, (int)B, (int)Ld, (int)cross, (int)q_batch,
                       static_cast<TO*>(dQ));
    FLMR_LAUNCH_CHECK();
    return FLMR_OK;
}

template <typename TQ, typename TO>
static int launch_grad_d(const void* Q, const int32_t* argmax, const float* G, int32_t q_batch, int32_t nq, int32_t B, int32_t Ld,
                         int32_t cross, void* dD, hipStream_t st) {
    hipLaunchKernelGGL((maxsim_grad_d_kernel<TQ, TO>), dim3((unsigned)flmr_ceil_div(Ld, SG_TILE), (unsigned)B), dim3(256), 0, st,
                       static_cast<const TQ*>(Q), argmax, G, (int)nq, (int)B, (int)Ld, (int)cross, (int)q_batch, static_cast<TO*>(dD));
    FLMR_LAUNCH_CHECK();
    return FLMR_OK;
}

// in_f16: the element type of the operand the kernel reads; out_f16: of the gradient it writes
#define SG_DISPATCH(fn, in_f16, out_f16, ...)                                              \
    ((in_f16) ? ((out_f16) ? fn<_Float16, _Float16>(__VA_ARGS__) : fn<_Float16, float>(__VA_ARGS__)) \
              : ((out_f16) ? fn<float, _Float16>(__VA_ARGS__) : fn<float, float>(__VA_ARGS__)))

static int maxsim_bwd(const void* Q, int32_t q_dtype, int32_t q_batch, int32_t nq, const void* D, int32_t d_dtype, int32_t B, int32_t Ld,
                      int32_t dim, int32_t cross, const int32_t* argmax, const float* grad_colmax, void* dQ, int32_t dq_dtype, void* dD,
                      int32_t dd_dtype, flmr_stream_t stream) {
    if (!Q || !D || !argmax || !grad_colmax) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    const int rc = flmr_maxsim_check(q_batch, B, cross, nq >= 1 && B >= 0 && Ld >= 0, 0, dim, nq, FLMR_MAXSIM_NQ_ANY);   // (no column state in LDS)
    if (rc) return rc;
    if (B > 65535 && dD) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "B=%d > 65535", B);
    if (B == 0) return FLMR_OK;
    if (cross && q_batch == 1) cross = 0;   // (the broadcast form: the same rows, the same sums)
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dQ) {
        const int rc = SG_DISPATCH(launch_grad_q, d_dtype == FLMR_F16, dq_dtype == FLMR_F16, D, argmax, grad_colmax, q_batch, nq, B, Ld, cross, dQ, st);
        if (rc) return rc;
    }
    if (dD && Ld > 0) {
        const int rc = SG_DISPATCH(launch_grad_d, q_dtype == FLMR_F16, dd_dtype == FLMR_F16, Q, argmax, grad_colmax, q_batch, nq, B, Ld, cross, dD, st);
        if (rc) return rc;
    }
    return FLMR_OK;
}

extern "C" int flmr_colbert_maxsim_bwd(const float* Q, int32_t q_batch, int32_t nq, const float* D, int32_t B, int32_t Ld,
                                       int32_t dim, int32_t cross, const int32_t* argmax, const float* grad_colmax, float* dQ,
                                       float* dD, flmr_stream_t stream) {
    return maxsim_bwd(Q, FLMR_F32, q_batch, nq, D, FLMR_F32, B, Ld, dim, cross, argmax, grad_colmax, dQ, FLMR_F32, dD, FLMR_F32, stream);
}

extern "C" int flmr_colbert_maxsim_bwd_typed(const void* Q, int32_t q_dtype, int32_t q_batch, int32_t nq, const void* D, int32_t d_dtype,
                                             int32_t B, int32_t Ld, int32_t dim, int32_t cross, const int32_t* argmax,
                                             const float* grad_colmax, void* dQ, int32_t dq_dtype, void* dD, int32_t dd_dtype,
                                             flmr_stream_t stream) {
    const int32_t dts[4] = {q_dtype, d_dtype, dq_dtype, dd_dtype};
    for (int k = 0; k < 4; k++)
        if (dts[k] != FLMR_F32 && dts[k] != FLMR_F16) FLMR_FAIL(FLMR_ERR_INVALID, "dtype=%d (FLMR_F32 or FLMR_F16)", dts[k]);
    // the typed ABI's own rules, ahead of the rest: alignment, and the forward's nq limit (nq < 1 is "bad sizes" below)
    const int rc = flmr_maxsim_check(1, 1, 0, true,
                                     reinterpret_cast<uintptr_t>(Q) | reinterpret_cast<uintptr_t>(D) | reinterpret_cast<uintptr_t>(dQ) | reinterpret_cast<uintptr_t>(dD),
                                     FLMR_DIM, nq > 0 ? nq : 0, FLMR_MAXSIM_NQ_KEYS);
    if (rc) return rc;
    if (q_dtype == FLMR_F16 && d_dtype == FLMR_F32 && dim == FLMR_DIM)
        FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "fp16 Q with fp32 D: widen Q and call the fp32 entry point");
    return maxsim_bwd(Q, q_dtype, q_batch, nq, D, d_dtype, B, Ld, dim, cross, argmax, grad_colmax, dQ, dq_dtype, dD, dd_dtype, stream);
}
