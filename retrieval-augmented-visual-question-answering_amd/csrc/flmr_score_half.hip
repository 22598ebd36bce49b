// The padded / cross MaxSim on HALF-PRECISION documents: flmr_colbert_score_typed, flmr_colbert_maxsim_fwd_typed and the dtype
// routing of flmr_colbert_maxsim_bwd_typed (include/flmr_hip.h).
//
// Every drop-in caller of the scoring head holds fp16 operands: ColBERT.doc() halves the documents (TPC/modeling/colbert.py:206)
// and colbert_score rounds the query to their dtype (:280-284).  The fp32 kernel (colbert_score_padded_mfma_kernel, flmr_ops.hip)
// would split such a value into fp16 hi / lo again with lo == +0 and spend three MFMAs per 16 dims where one carries all the
// information.  The kernel here reads the fp16 rows as they are and issues only the products whose operands can be non-zero:
//   D fp16, Q fp16:  hi(D) x hi(Q)                       one MFMA per 16 dims, Q staged as it is (hi plane only: half the LDS)
//   D fp16, Q fp32:  hi(D) x hi(Q), hi(D) x lo(Q)        two MFMAs; fp32 Q split while it is staged, in BOTH instantiations
// Neither form has a workspace or a host synchronisation.  A skipped accumulator enters the epilogue as the +0.0f the fp32 kernel
// accumulates from all-zero low parts, so out / colmax / argmax are bit-identical to the fp32 entry points on the widened operands
// (tests/test_score_half_gpu.py, torch.equal).
// TWIN: colbert_score_padded_mfma_kernel (flmr_ops.hip) and maxsim_gather_fwd_kernel (flmr_rescore.hip) -- the tile walk, the
// accumulator-row -> token mapping, the (f2ord(v) << 32 | ~token) key, the tie rule and the epilogue order here are theirs; a fix
// to any of them must be made in all three.  They are copies, not one template: the search-side scorer keeps its register
// allocation.
#include "flmr_device.h"

typedef _Float16 sh8 __attribute__((ext_vector_type(8)));
#define SH_QC 4        // query tiles of 32 rows staged per pass (as PS_QC)
#define SH_BROW 136    // LDS row pitch in halves (as PS_BROW)

template <bool QF16>
static constexpr size_t sh_stage_bytes() { return (size_t)SH_QC * (QF16 ? 1 : 2) * 32 * SH_BROW * sizeof(_Float16); }

// One workgroup per document (x query in the cross form, gridDim.y > 1), the 4 waves walk the document's 32-token tiles; query
// chunks of SH_QC x 32 rows are staged in LDS and shared by the waves.  Q is [rows, nq, 128] in its own element type.
template <bool ARGMAX, bool QF16>
__global__ __launch_bounds__(256, 2) void colbert_score_half_kernel(const void* __restrict__ Qv, int q_batch, int nq, int nqp,
                                                                    const _Float16* __restrict__ D,
                                                                    const uint8_t* __restrict__ mask, int Ld, float* out,
                                                                    float* colmax_out, int32_t* argmax_out) {
    constexpr int PL = QF16 ? 1 : 2;   // staged planes per query tile: hi | hi, lo
    extern __shared__ __attribute__((aligned(16))) char smem[];
    _Float16* bq = reinterpret_cast<_Float16*>(smem);                                          // [SH_QC][PL][32][SH_BROW]
    unsigned int* colmax = reinterpret_cast<unsigned int*>(bq + SH_QC * PL * 32 * SH_BROW);    // [nqp] order-preserving fp32 image
    unsigned long long* colkey = reinterpret_cast<unsigned long long*>(colmax);                 // ARGMAX: [nqp] (value, ~token)
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, h = lane >> 5;
    const size_t ob = (size_t)blockIdx.y * gridDim.x + b;
    const size_t qrow0 = (gridDim.y > 1 ? (size_t)blockIdx.y : (q_batch == 1 ? 0 : (size_t)b)) * nq;
    for (int k = tid; k < nqp; k += 256) {  // below every real value
        if constexpr (ARGMAX) colkey[k] = 0ull;
        else colmax[k] = 0u;
    }
    const int ntiles = (Ld + 31) >> 5;
    for (int qc0 = 0; qc0 < nq; qc0 += 32 * SH_QC) {
        const int ntq = ((nq - qc0 < 32 * SH_QC ? nq - qc0 : 32 * SH_QC) + 31) >> 5;
        __syncthreads();
        for (int e = tid; e < ntq * 512; e += 256) {   // rows >= nq stage as zero (score_split_q's rule)
            const int piece = e & 15, row = (e >> 4) & 31, qt = e >> 9, r = qc0 + qt * 32 + row;
            if constexpr (QF16) {
                sh8 hi8;
                if (r < nq) {
                    hi8 = *reinterpret_cast<const sh8*>(static_cast<const _Float16*>(Qv) + (qrow0 + r) * FLMR_DIM + piece * 8);
                } else {
#pragma unroll
                    for (int k = 0; k < 8; k++) hi8[k] = (_Float16)0.0f;
                }
                *reinterpret_cast<sh8*>(bq + (qt * 32 + row) * SH_BROW + piece * 8) = hi8;
            } else {   // fp32 Q split on the fly: the hi / lo values score_split_q writes
                sh8 hi8, lo8;
                if (r < nq) {
                    const float4* src = reinterpret_cast<const float4*>(static_cast<const float*>(Qv) + (qrow0 + r) * FLMR_DIM + piece * 8);
                    const float4 x = src[0], y = src[1];
                    const float v[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
#pragma unroll
                    for (int k = 0; k < 8; k++) {
                        const _Float16 hi = (_Float16)v[k];
                        hi8[k] = hi;
                        lo8[k] = (_Float16)((v[k] - (float)hi) * 2048.0f);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 8; k++) { hi8[k] = (_Float16)0.0f; lo8[k] = (_Float16)0.0f; }
                }
                *reinterpret_cast<sh8*>(bq + ((qt * 2 + 0) * 32 + row) * SH_BROW + piece * 8) = hi8;
                *reinterpret_cast<sh8*>(bq + ((qt * 2 + 1) * 32 + row) * SH_BROW + piece * 8) = lo8;
            }
        }
        __syncthreads();
        for (int t = wave; t < ntiles; t += 4) {
            const int tok = t * 32 + i;
            const bool inb = tok < Ld;
            sh8 ah[8];   // the fp16 row IS the hi operand; its lo part is +0 and is never formed
            {
                const sh8* p = reinterpret_cast<const sh8*>(D + ((size_t)b * Ld + (inb ? tok : 0)) * FLMR_DIM + 64 * h);   // (rows past Ld re-read token 0)
#pragma unroll
                for (int s = 0; s < 8; s++) ah[s] = p[s];
            }
            // which of this lane's 16 accumulator rows are real, unmasked tokens (bit r)
            uint32_t okbits = 0;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (row < Ld && mask[(size_t)b * Ld + row]) okbits |= 1u << r;
            }
            for (int qt = 0; qt < ntq; qt++) {
                f32x16 acch, accl;
#pragma unroll
                for (int r = 0; r < 16; r++) { acch[r] = 0.0f; accl[r] = 0.0f; }
#pragma unroll
                for (int s = 0; s < 8; s++) {
                    const sh8 bh = *reinterpret_cast<const sh8*>(bq + ((qt * PL + 0) * 32 + i) * SH_BROW + 64 * h + 8 * s);
                    acch = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s], bh, acch, 0, 0, 0);
                    if constexpr (!QF16) {
                        const sh8 bl = *reinterpret_cast<const sh8*>(bq + ((qt * PL + 1) * 32 + i) * SH_BROW + 64 * h + 8 * s);
                        accl = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s], bl, accl, 0, 0, 0);
                    }
                }
                float mx = FLMR_NEG_INF;
                int arg = 0x7fffffff;   // ARGMAX: the lowest row holding mx (rows ascend with r for a fixed h)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int row = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    // the fp32 kernel's fmaf(accl + accm, 2^-11, acch): accm (and, for fp16 Q, accl) is the +0 it accumulates from
                    // all-zero low parts
                    const float v = ((okbits >> r) & 1u) ? fmaf(accl[r] + 0.0f, 1.0f / 2048.0f, acch[r]) : -9999.0f;  // colbert.py:240
                    if constexpr (ARGMAX) {
                        if (row < Ld && v > mx) { mx = v; arg = row; }
                    } else {
                        if (row < Ld) mx = fmaxf(mx, v);
                    }
                }
                const int col = qc0 + qt * 32 + i;
                if constexpr (ARGMAX) {
                    const float omx = __shfl_xor(mx, 32, 64);
                    const int oarg = __shfl_xor(arg, 32, 64);
                    if (omx > mx || (omx == mx && oarg < arg)) { mx = omx; arg = oarg; }
                    if (h == 0 && col < nq && mx > FLMR_NEG_INF)
                        atomicMax(&colkey[col], ((unsigned long long)flmr_f2ord(mx) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)arg));
                } else {
                    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                    if (h == 0 && col < nq && mx > FLMR_NEG_INF) atomicMax(&colmax[col], flmr_f2ord(mx));
                }
            }
        }
    }
    __syncthreads();
    auto cmax = [&](int k) -> float {
        if constexpr (ARGMAX) return (Ld > 0) ? flmr_ord2f((unsigned int)(colkey[k] >> 32)) : FLMR_NEG_INF;
        else return (Ld > 0) ? flmr_ord2f(colmax[k]) : FLMR_NEG_INF;
    };
    if constexpr (ARGMAX)
        for (int k = tid; k < nq; k += 256) {
            const int tok = (Ld > 0) ? (int)(0xFFFFFFFFu - (uint32_t)colkey[k]) : -1;
            argmax_out[ob * nq + k] = (tok >= 0 && mask[(size_t)b * Ld + tok]) ? tok : -1;
        }
    if (colmax_out)
        for (int k = tid; k < nq; k += 256) colmax_out[ob * nq + k] = cmax(k);
    if (tid == 0 && out) {
        float sc = 0.0f;
        for (int k = 0; k < nq; k++) sc += cmax(k);
        out[ob] = sc;
    }
}

// ---- entry points ---------------------------------------------------------------------------------------------------------
static bool sh_dtype_ok(int32_t t) { return t == FLMR_F32 || t == FLMR_F16; }

// the checks every typed entry point shares; *launch = false: B == 0, nothing to do
static int sh_check(const void* Q, int32_t q_dtype, int32_t q_batch, int32_t nq, const void* D, int32_t d_dtype, int32_t B, int32_t Ld,
                    int32_t dim, int32_t cross, bool* launch) {
    *launch = false;
    if (!sh_dtype_ok(q_dtype) || !sh_dtype_ok(d_dtype)) FLMR_FAIL(FLMR_ERR_INVALID, "q_dtype=%d d_dtype=%d (FLMR_F32 or FLMR_F16)", q_dtype, d_dtype);
    if (!Q || !D) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    if (!cross && q_batch != 1 && q_batch != B) FLMR_FAIL(FLMR_ERR_INVALID, "q_batch must be 1 or B");
    if (cross && (q_batch < 1 || q_batch > 65535)) FLMR_FAIL(FLMR_ERR_INVALID, "cross scoring takes 1..65535 queries per call");
    if (nq < 1 || B < 0 || Ld < 0) FLMR_FAIL(FLMR_ERR_INVALID, "bad sizes");
    if ((reinterpret_cast<uintptr_t>(Q) | reinterpret_cast<uintptr_t>(D)) & 15) FLMR_FAIL(FLMR_ERR_INVALID, "Q and D must be 16-byte aligned");
    if (dim != FLMR_DIM) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "dim=%d (this build: %d)", dim, FLMR_DIM);
    if ((size_t)nq * 8 > 64 * 1024) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "nq=%d too large", nq);
    if (q_dtype == FLMR_F16 && d_dtype == FLMR_F32)
        FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "fp16 Q with fp32 D: widen Q and call the fp32 entry point");
    *launch = B > 0;
    return FLMR_OK;
}

template <bool ARGMAX, bool QF16>
static int sh_launch(const void* Q, int32_t q_batch, int32_t nq, const void* D, const uint8_t* mask, int32_t B, int32_t Ld, int32_t cross,
                     float* out, float* colmax, int32_t* argmax, hipStream_t st) {
    const dim3 grid((unsigned)B, cross ? (unsigned)q_batch : 1u);
    const int nqp = (int)flmr_round_up(nq, 32);
    const size_t lds = sh_stage_bytes<QF16>() + (size_t)nqp * (ARGMAX ? sizeof(unsigned long long) : sizeof(unsigned int));
    FLMR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(colbert_score_half_kernel<ARGMAX, QF16>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((colbert_score_half_kernel<ARGMAX, QF16>), grid, dim3(256), lds, st, Q, (int)q_batch, (int)nq, nqp,
                       static_cast<const _Float16*>(D), mask, (int)Ld, out, colmax, argmax);
    FLMR_LAUNCH_CHECK();
    return FLMR_OK;
}

extern "C" int flmr_colbert_score_typed(const void* Q, int32_t q_dtype, int32_t q_batch, int32_t nq, const void* D, int32_t d_dtype,
                                        const uint8_t* mask, int32_t B, int32_t Ld, int32_t dim, int32_t cross, float* out,
                                        float* colmax, flmr_stream_t stream) {
    bool launch;
    const int rc = sh_check(Q, q_dtype, q_batch, nq, D, d_dtype, B, Ld, dim, cross, &launch);
    if (rc) return rc;
    if (!mask || (!out && !colmax)) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    if (!launch) return FLMR_OK;
    if (d_dtype == FLMR_F32) {   // (F32, F32): the fp32 scorer, one call per requested output
        const float *Qf = static_cast<const float*>(Q), *Df = static_cast<const float*>(D);
        if (out) {
            const int r = cross ? flmr_colbert_score_cross(Qf, q_batch, nq, Df, mask, B, Ld, dim, out, stream)
                                : flmr_colbert_score_padded(Qf, q_batch, nq, Df, mask, B, Ld, dim, out, stream);
            if (r) return r;
        }
        if (colmax) {
            if (cross && q_batch != 1) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "the fp32 forward-only scorer has no cross column maxima");
            return flmr_colbert_colmax_padded(Qf, q_batch, nq, Df, mask, B, Ld, dim, colmax, stream);
        }
        return FLMR_OK;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (q_dtype == FLMR_F16) return sh_launch<false, true>(Q, q_batch, nq, D, mask, B, Ld, cross, out, colmax, nullptr, st);
    return sh_launch<false, false>(Q, q_batch, nq, D, mask, B, Ld, cross, out, colmax, nullptr, st);
}

extern "C" int flmr_colbert_maxsim_fwd_typed(const void* Q, int32_t q_dtype, int32_t q_batch, int32_t nq, const void* D,
                                             int32_t d_dtype, const uint8_t* mask, int32_t B, int32_t Ld, int32_t dim, int32_t cross,
                                             float* out, float* colmax, int32_t* argmax, flmr_stream_t stream) {
    bool launch;
    const int rc = sh_check(Q, q_dtype, q_batch, nq, D, d_dtype, B, Ld, dim, cross, &launch);
    if (rc) return rc;
    if (!mask || !argmax) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    if (!launch) return FLMR_OK;
    if (d_dtype == FLMR_F32)
        return flmr_colbert_maxsim_fwd(static_cast<const float*>(Q), q_batch, nq, static_cast<const float*>(D), mask, B, Ld, dim, cross,
                                       out, colmax, argmax, stream);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (q_dtype == FLMR_F16) return sh_launch<true, true>(Q, q_batch, nq, D, mask, B, Ld, cross, out, colmax, argmax, st);
    return sh_launch<true, false>(Q, q_batch, nq, D, mask, B, Ld, cross, out, colmax, argmax, st);
}
