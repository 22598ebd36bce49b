// Retrieve-and-rescore for RAG training (src/models/rag/rag_model_blip.py:409-442): the GATHERED forms of the padded MaxSim
// under autograd, flmr_maxsim_gather_fwd / _bwd.
//
// Output row r = q * k + j scores query q against passage pids[q, j] of a device-resident store [npassages, Ld, 128] (fp32 or
// fp16) with mask [npassages, Ld].  The forward is colbert_score_padded_mfma_kernel<true> (flmr_ops.hip) with the document base
// taken from the pid and the query block from r / k: the same staging of Q, the same tile walk, the same accumulation and the
// same (value, ~token) LDS key, so out / colmax / argmax are bit-identical to flmr_colbert_maxsim_fwd on
// Q.repeat_interleave(k) and store[pids] -- neither of which is ever built.  An fp16 store value has a zero low part, so the
// third product of the split (lo(D) x hi(Q)) is identically +0 and is not issued: two MFMAs per 16 dims instead of three and
// half the bytes per token row, with the same bits as the fp32 kernel gives the widened values.
// The backward writes dQ alone (the store is a constant of training): one wave per (q, i), the k rows of the query walked in
// ascending j -- a fixed order, no floating-point atomics.
#include "flmr_device.h"

typedef _Float16 rh8 __attribute__((ext_vector_type(8)));
typedef _Float16 rh2 __attribute__((ext_vector_type(2)));
#define RS_QC 4        // query tiles of 32 rows staged per pass (as PS_QC)
#define RS_BROW 136    // LDS row pitch in halves (as PS_BROW)

template <bool F16>
__global__ __launch_bounds__(256, 2) void maxsim_gather_fwd_kernel(const float* __restrict__ Qf, int nq, int nqp,
                                                                   const void* __restrict__ store,
                                                                   const uint8_t* __restrict__ store_mask, int npassages, int Ld,
                                                                   const int32_t* __restrict__ pids, int k,
                                                                   float* out, float* colmax_out, int32_t* argmax_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    _Float16* bq = reinterpret_cast<_Float16*>(smem);                                                   // [RS_QC][hi|lo][32][RS_BROW]
    unsigned long long* colkey = reinterpret_cast<unsigned long long*>(bq + RS_QC * 2 * 32 * RS_BROW);   // [nqp] (value, ~token)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, h = lane >> 5;
    const size_t ob = blockIdx.x;
    const size_t qrow0 = (ob / (size_t)k) * nq;
    const int pid = pids[ob];
    // an empty slot is an all-padded document: every token scores -9999, nothing is read (a pid past the store, the caller's
    // error, is kept from reading out of bounds the same way)
    const bool live = pid >= 0 && pid < npassages;
    const uint8_t* mrow = store_mask + (size_t)(live ? pid : 0) * Ld;
    // what the tile walk leaves in a column of an all-padded document: -9999 held by token 0
    const unsigned long long padkey = ((unsigned long long)flmr_f2ord(-9999.0f) << 32) | 0xFFFFFFFFull;
    for (int c = tid; c < nqp; c += 256) colkey[c] = (!live && Ld > 0 && c < nq) ? padkey : 0ull;
    const int ntiles = live ? (Ld + 31) >> 5 : 0;
    for (int qc0 = 0; qc0 < nq && live; qc0 += 32 * RS_QC) {
        const int ntq = ((nq - qc0 < 32 * RS_QC ? nq - qc0 : 32 * RS_QC) + 31) >> 5;
        __syncthreads();
        for (int e = tid; e < ntq * 512; e += 256) {   // fp32 Q split on the fly; rows >= nq stage as zero
            const int piece = e & 15, row = (e >> 4) & 31, qt = e >> 9, r = qc0 + qt * 32 + row;
            rh8 hi8, lo8;
            if (r < nq) {
                const float4* src = reinterpret_cast<const float4*>(Qf + (qrow0 + r) * FLMR_DIM + piece * 8);
                const float4 x = src[0], y = src[1];
                const float v[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
#pragma unroll
                for (int d = 0; d < 8; d++) {
                    const _Float16 hi = (_Float16)v[d];
                    hi8[d] = hi;
                    lo8[d] = (_Float16)((v[d] - (float)hi) * 2048.0f);
                }
            } else {
#pragma unroll
                for (int d = 0; d < 8; d++) { hi8[d] = (_Float16)0.0f; lo8[d] = (_Float16)0.0f; }
            }
            *reinterpret_cast<rh8*>(bq + ((qt * 2 + 0) * 32 + row) * RS_BROW + piece * 8) = hi8;
            *reinterpret_cast<rh8*>(bq + ((qt * 2 + 1) * 32 + row) * RS_BROW + piece * 8) = lo8;
        }
        __syncthreads();
        for (int t = wave; t < ntiles; t += 4) {
            const int tok = t * 32 + i;
            const size_t drow = ((size_t)pid * Ld + (tok < Ld ? tok : 0)) * FLMR_DIM + 64 * h;   // (rows past Ld re-read token 0)
            rh8 ah[8], al[8];
            if constexpr (F16) {
                const rh8* p = reinterpret_cast<const rh8*>(reinterpret_cast<const _Float16*>(store) + drow);
#pragma unroll
                for (int s = 0; s < 8; s++) ah[s] = p[s];
            } else {
                const float4* p = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(store) + drow);
#pragma unroll
                for (int s = 0; s < 8; s++) {
                    const float4 x = p[2 * s], y = p[2 * s + 1];
                    const float v[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const _Float16 hi = (_Float16)v[e];
                        ah[s][e] = hi;
                        al[s][e] = (_Float16)((v[e] - (float)hi) * 2048.0f);
                    }
                }
            }
            uint32_t okbits = 0;   // which of this lane's 16 accumulator rows are real, unmasked tokens (bit r)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (row < Ld && mrow[row]) okbits |= 1u << r;
            }
            for (int qt = 0; qt < ntq; qt++) {
                f32x16 acch, accl, accm;
#pragma unroll
                for (int r = 0; r < 16; r++) { acch[r] = 0.0f; accl[r] = 0.0f; accm[r] = 0.0f; }
#pragma unroll
                for (int s = 0; s < 8; s++) {
                    const rh8 bh = *reinterpret_cast<const rh8*>(bq + ((qt * 2 + 0) * 32 + i) * RS_BROW + 64 * h + 8 * s);
                    const rh8 bl = *reinterpret_cast<const rh8*>(bq + ((qt * 2 + 1) * 32 + i) * RS_BROW + 64 * h + 8 * s);
                    acch = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s], bh, acch, 0, 0, 0);
                    accl = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s], bl, accl, 0, 0, 0);
                    if constexpr (!F16) accm = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[s], bh, accm, 0, 0, 0);
                }
                float mx = FLMR_NEG_INF;
                int arg = 0x7fffffff;   // the lowest row holding mx (rows ascend with r for a fixed h)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int row = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    // fp16 store: accm is the +0 the fp32 kernel accumulates from all-zero low parts
                    const float v = ((okbits >> r) & 1u) ? fmaf(accl[r] + accm[r], 1.0f / 2048.0f, acch[r]) : -9999.0f;  // colbert.py:240
                    if (row < Ld && v > mx) { mx = v; arg = row; }
                }
                const int col = qc0 + qt * 32 + i;
                const float omx = __shfl_xor(mx, 32, 64);
                const int oarg = __shfl_xor(arg, 32, 64);
                if (omx > mx || (omx == mx && oarg < arg)) { mx = omx; arg = oarg; }
                if (h == 0 && col < nq && mx > FLMR_NEG_INF)
                    atomicMax(&colkey[col], ((unsigned long long)flmr_f2ord(mx) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)arg));
            }
        }
    }
    __syncthreads();
    auto cmax = [&](int c) -> float { return (Ld > 0) ? flmr_ord2f((unsigned int)(colkey[c] >> 32)) : FLMR_NEG_INF; };
    for (int c = tid; c < nq; c += 256) {
        const int tok = (Ld > 0) ? (int)(0xFFFFFFFFu - (uint32_t)colkey[c]) : -1;
        argmax_out[ob * nq + c] = (live && tok >= 0 && mrow[tok]) ? tok : -1;
    }
    if (colmax_out)
        for (int c = tid; c < nq; c += 256) colmax_out[ob * nq + c] = cmax(c);
    if (tid == 0 && out) {
        float sc = 0.0f;
        for (int c = 0; c < nq; c++) sc += cmax(c);
        out[ob] = sc;
    }
}

// one wave per (query q, column i); lane l owns dims 2l, 2l+1; the k rows of the query 64 at a time, added in ascending j
template <bool F16>
__global__ __launch_bounds__(256) void maxsim_gather_grad_q_kernel(const void* __restrict__ store, int npassages, int Ld,
                                                                   const int32_t* __restrict__ pids, int nqueries, int k, int nq,
                                                                   const int32_t* __restrict__ argmax, const float* __restrict__ G,
                                                                   float* __restrict__ dQ) {
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= (int64_t)nqueries * nq) return;
    const int q = (int)(pair / nq), i = (int)(pair % nq);
    float2 acc = make_float2(0.0f, 0.0f);
    for (int j0 = 0; j0 < k; j0 += 64) {
        const int jj = j0 + lane;
        int a_l = -1, p_l = -1;
        float g_l = 0.0f;
        if (jj < k) {
            const size_t r = (size_t)q * k + jj;
            a_l = argmax[r * nq + i];
            g_l = G[r * nq + i];
            p_l = pids[r];
        }
        const int n = k - j0 < 64 ? k - j0 : 64;
        for (int j = 0; j < n; j++) {
            const int a = __shfl(a_l, j, 64);
            const int p = __shfl(p_l, j, 64);
            const float g = __shfl(g_l, j, 64);
            if (a < 0 || a >= Ld || p < 0 || p >= npassages) continue;
            const size_t off = ((size_t)p * Ld + a) * FLMR_DIM + 2 * lane;
            float2 d;
            if constexpr (F16) {
                const rh2 hv = *reinterpret_cast<const rh2*>(reinterpret_cast<const _Float16*>(store) + off);
                d = make_float2((float)hv[0], (float)hv[1]);
            } else {
                d = *reinterpret_cast<const float2*>(reinterpret_cast<const float*>(store) + off);
            }
            acc.x = fmaf(g, d.x, acc.x);
            acc.y = fmaf(g, d.y, acc.y);
        }
    }
    *reinterpret_cast<float2*>(dQ + (size_t)pair * FLMR_DIM + 2 * lane) = acc;
}

static int gather_sizes(int32_t store_dtype, int32_t npassages, int32_t Ld, int32_t dim, int32_t nqueries, int32_t k, int32_t nq) {
    if (store_dtype != FLMR_F32 && store_dtype != FLMR_F16) FLMR_FAIL(FLMR_ERR_INVALID, "store_dtype=%d (FLMR_F32 or FLMR_F16)", store_dtype);
    if (nq < 1 || nqueries < 0 || k < 0 || npassages < 0 || Ld < 0) FLMR_FAIL(FLMR_ERR_INVALID, "bad sizes");
    if (dim != FLMR_DIM) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "dim=%d (this build: %d)", dim, FLMR_DIM);
    if ((size_t)nq * 8 > 64 * 1024) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "nq=%d too large", nq);
    if ((int64_t)nqueries * k > 0x7fffffffll) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "nqueries * k = %lld rows", (long long)nqueries * k);
    return FLMR_OK;
}

extern "C" int flmr_maxsim_gather_fwd(const float* Q, int32_t nqueries, int32_t nq, const void* store, int32_t store_dtype,
                                      const uint8_t* store_mask, int32_t npassages, int32_t Ld, int32_t dim, const int32_t* pids,
                                      int32_t k, float* out, float* colmax, int32_t* argmax, flmr_stream_t stream) {
    const int rc = gather_sizes(store_dtype, npassages, Ld, dim, nqueries, k, nq);
    if (rc) return rc;
    if ((int64_t)nqueries * k == 0) return FLMR_OK;
    if (!Q || !pids || !argmax) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    if ((int64_t)npassages * Ld > 0 && (!store || !store_mask)) FLMR_FAIL(FLMR_ERR_INVALID, "NULL store");
    if ((reinterpret_cast<uintptr_t>(store) | reinterpret_cast<uintptr_t>(Q)) & 15) FLMR_FAIL(FLMR_ERR_INVALID, "Q and store must be 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int nqp = (int)((nq + 31) / 32 * 32);
    const size_t lds = (size_t)RS_QC * 2 * 32 * RS_BROW * sizeof(_Float16) + (size_t)nqp * sizeof(unsigned long long);
    const dim3 grid((unsigned)((int64_t)nqueries * k));
    if (store_dtype == FLMR_F16) {
        FLMR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(maxsim_gather_fwd_kernel<true>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(maxsim_gather_fwd_kernel<true>, grid, dim3(256), lds, st, Q, (int)nq, nqp, store, store_mask, (int)npassages, (int)Ld, pids,
                           (int)k, out, colmax, argmax);
    } else {
        FLMR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(maxsim_gather_fwd_kernel<false>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(maxsim_gather_fwd_kernel<false>, grid, dim3(256), lds, st, Q, (int)nq, nqp, store, store_mask, (int)npassages, (int)Ld, pids,
                           (int)k, out, colmax, argmax);
    }
    FLMR_LAUNCH_CHECK();
    return FLMR_OK;
}

extern "C" int flmr_maxsim_gather_bwd(const void* store, int32_t store_dtype, int32_t npassages, int32_t Ld, int32_t dim,
                                      const int32_t* pids, int32_t nqueries, int32_t k, int32_t nq, const int32_t* argmax,
                                      const float* grad_colmax, float* dQ, flmr_stream_t stream) {
    const int rc = gather_sizes(store_dtype, npassages, Ld, dim, nqueries, k, nq);
    if (rc) return rc;
    if ((int64_t)nqueries * k == 0) return FLMR_OK;   // (nothing is launched: dQ is the caller's to zero)
    if (!dQ || !pids || !argmax || !grad_colmax) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    if ((int64_t)npassages * Ld > 0 && !store) FLMR_FAIL(FLMR_ERR_INVALID, "NULL store");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t pairs = (int64_t)nqueries * nq;
    const dim3 grid((unsigned)flmr_ceil_div(pairs, 4));
    if (store_dtype == FLMR_F16)
        hipLaunchKernelGGL(maxsim_gather_grad_q_kernel<true>, grid, dim3(256), 0, st, store, (int)npassages, (int)Ld, pids, (int)nqueries, (int)k, (int)nq,
                           argmax, grad_colmax, dQ);
    else
        hipLaunchKernelGGL(maxsim_gather_grad_q_kernel<false>, grid, dim3(256), 0, st, store, (int)npassages, (int)Ld, pids, (int)nqueries, (int)k, (int)nq,
                           argmax, grad_colmax, dQ);
    FLMR_LAUNCH_CHECK();
    return FLMR_OK;
}
