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
// The tile body (staging, row mapping, products, fold, key, epilogue) is flmr_maxsim_tile.h's, shared with
// colbert_score_padded_mfma_kernel (flmr_ops.hip) and maxsim_gather_fwd_kernel (flmr_rescore.hip); the kernels stay separate so
// that the search-side scorer keeps its register allocation.
#include "flmr_maxsim_tile.h"

// One workgroup per document (x query in the cross form, gridDim.y > 1), the 4 waves walk the document's 32-token tiles; query
// chunks of MT_QC x 32 rows are staged in LDS and shared by the waves.  Q is [rows, nq, 128] in its own element type.
template <bool ARGMAX, bool QF16>
__global__ __launch_bounds__(256, 2) void colbert_score_half_kernel(const void* __restrict__ Qv, int q_batch, int nq, int nqp,
                                                                    const _Float16* __restrict__ D,
                                                                    const uint8_t* __restrict__ mask, int Ld, float* out,
                                                                    float* colmax_out, int32_t* argmax_out) {
    constexpr int PL = QF16 ? 1 : 2;   // staged planes per query tile: hi | hi, lo
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const mt_lds<PL, mt_col_t<ARGMAX>> L{nqp};
    _Float16* bq = reinterpret_cast<_Float16*>(smem + L.bq);
    mt_col_t<ARGMAX>* cols = reinterpret_cast<mt_col_t<ARGMAX>*>(smem + L.cols);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, h = lane >> 5;
    const size_t ob = (size_t)blockIdx.y * gridDim.x + b;
    const size_t qrow0 = (gridDim.y > 1 ? (size_t)blockIdx.y : (q_batch == 1 ? 0 : (size_t)b)) * nq;
    for (int k = tid; k < nqp; k += 256) cols[k] = 0;   // below every real value
    const int ntiles = (Ld + 31) >> 5;
    for (int qc0 = 0; qc0 < nq; qc0 += 32 * MT_QC) {
        const int ntq = mt_chunk_tiles(nq, qc0);
        __syncthreads();
        if constexpr (QF16) mt_stage_q_f16(bq, static_cast<const _Float16*>(Qv), qrow0, qc0, ntq, nq, tid);
        else mt_stage_q_f32(bq, static_cast<const float*>(Qv), qrow0, qc0, ntq, nq, tid);   // fp32 Q split on the fly
        __syncthreads();
        for (int t = wave; t < ntiles; t += 4) {
            const int tok = t * 32 + i;
            const bool inb = tok < Ld;
            f16x8 ah[8];
            mt_load_row_f16(D + ((size_t)b * Ld + (inb ? tok : 0)) * FLMR_DIM + 64 * h, ah);   // (rows past Ld re-read token 0)
            uint32_t okbits = 0;   // which of this lane's 16 accumulator rows are real, unmasked tokens (bit r)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = mt_row(t, r, h);
                if (row < Ld && mask[(size_t)b * Ld + row]) okbits |= 1u << r;
            }
            for (int qt = 0; qt < ntq; qt++) {
                f32x16 acch, accl, accm;
                mt_products<!QF16, false>(bq, qt, i, h, ah, ah, acch, accl, accm);   // (no low part of D: the `al` argument is not read)
                mt_fold<ARGMAX>(acch, accl, accm, okbits, t, h, Ld, qc0 + qt * 32 + i, nq, cols);
            }
        }
    }
    __syncthreads();
    mt_epilogue<ARGMAX>(cols, Ld > 0, [=](int tok) { return mask[(size_t)b * Ld + tok]; }, ob, nq, tid, out, colmax_out, argmax_out);
}

// ---- entry points ---------------------------------------------------------------------------------------------------------
static bool sh_dtype_ok(int32_t t) { return t == FLMR_F32 || t == FLMR_F16; }

// the checks every typed entry point shares; *launch = false: B == 0, nothing to do
static int sh_check(const void* Q, int32_t q_dtype, int32_t q_batch, int32_t nq, const void* D, int32_t d_dtype, int32_t B, int32_t Ld,
                    int32_t dim, int32_t cross, bool* launch) {
    *launch = false;
    if (!sh_dtype_ok(q_dtype) || !sh_dtype_ok(d_dtype)) FLMR_FAIL(FLMR_ERR_INVALID, "q_dtype=%d d_dtype=%d (FLMR_F32 or FLMR_F16)", q_dtype, d_dtype);
    if (!Q || !D) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    const int rc = flmr_maxsim_check(q_batch, B, cross, nq >= 1 && B >= 0 && Ld >= 0, reinterpret_cast<uintptr_t>(Q) | reinterpret_cast<uintptr_t>(D),
                                     dim, nq, FLMR_MAXSIM_NQ_KEYS);
    if (rc) return rc;
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
    const size_t lds = mt_lds<(QF16 ? 1 : 2), mt_col_t<ARGMAX>>{nqp}.bytes;
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
