// The tile body of the padded MaxSim forward, shared by its three kernels:
//   colbert_score_padded_mfma_kernel<ARGMAX>   flmr_ops.hip         fp32 documents [B, Ld, 128] + mask
//   maxsim_gather_fwd_kernel<L>                flmr_rescore.hip     documents picked by pid through a loader (store / index)
//   colbert_score_half_kernel<ARGMAX, QF16>    flmr_score_half.hip  fp16 documents, fp16 or fp32 queries
// One workgroup of 4 waves per output row; query chunks of MT_QC x 32 rows are staged in LDS as fp16 hi (| lo) planes, every wave
// walks 32-token tiles of the document, contracts a tile with each staged query tile by v_mfma_f32_32x32x16_f16 on the fp16
// hi / lo split (hi.hi + 2^-11 (hi.lo + lo.hi), fp32 accumulation) and folds the 32x32 result into the LDS column state.
// The kernels stay three (the search-side scorer keeps its register allocation): they own the launch geometry,
// the LDS layout, the barriers and the document source; the arithmetic, the row mapping, the key and the tie rule are here, once.
#pragma once
#include "flmr_device.h"
#include <type_traits>

#define MT_QC 4        // query tiles of 32 rows staged per pass
#define MT_BROW 136    // LDS row pitch in halves

// The three kernels' dynamic LDS: the staged query planes (PL = 2: hi | lo; 1: hi only), the column state (COL = mt_col_t<ARGMAX>)
// and, behind it, `table` bytes of the document loader's own (the gathered kernel's decode table; 16-byte aligned: nqp % 32 == 0)
template <int PL, class COL>
struct mt_lds {
    int nqp;
    size_t table = 0;
    flmr_lds c;
    size_t bq = c.take<_Float16>(MT_QC * PL * 32 * MT_BROW);   // [MT_QC][PL][32][MT_BROW]
    size_t cols = c.take<COL>(nqp);                            // [nqp] column state
    size_t ltab = c.take<char>(table);
    size_t bytes = c.bytes;
};
static_assert(mt_lds<2, unsigned int>{32}.bytes == 69760 && mt_lds<2, unsigned long long>{32}.bytes == 69888 &&
              mt_lds<1, unsigned int>{32}.bytes == 34944 && mt_lds<2, unsigned long long>{32, 4096}.bytes == 73984, "padded MaxSim kernels' dynamic LDS at one query tile");
// query tiles of the chunk that starts at row qc0
__device__ __forceinline__ int mt_chunk_tiles(int nq, int qc0) { return ((nq - qc0 < 32 * MT_QC ? nq - qc0 : 32 * MT_QC) + 31) >> 5; }

// ---- the fp16 split ------------------------------------------------------------------------------------------------------
// 8 fp32 values -> fp16 hi / lo (lo scaled by 2^11): the values score_split_q writes
__device__ __forceinline__ void mt_split8(const float (&v)[8], f16x8& hi8, f16x8& lo8) {
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const _Float16 hi = (_Float16)v[k];
        hi8[k] = hi;
        lo8[k] = (_Float16)((v[k] - (float)hi) * 2048.0f);
    }
}
__device__ __forceinline__ void mt_split8(const float4* src, f16x8& hi8, f16x8& lo8) {
    const float4 x = src[0], y = src[1];
    const float v[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
    mt_split8(v, hi8, lo8);
}
// 64 dims of an fp32 row (the lane's half row) as hi / lo MFMA A fragments
__device__ __forceinline__ void mt_load_row_f32(const float* row, f16x8 (&ah)[8], f16x8 (&al)[8]) {
    const float4* p = reinterpret_cast<const float4*>(row);
#pragma unroll
    for (int s = 0; s < 8; s++) mt_split8(p + 2 * s, ah[s], al[s]);
}
// the same of an fp16 row: it IS the hi operand; its lo part is +0 and is never formed
__device__ __forceinline__ void mt_load_row_f16(const _Float16* row, f16x8 (&ah)[8]) {
    const f16x8* p = reinterpret_cast<const f16x8*>(row);
#pragma unroll
    for (int s = 0; s < 8; s++) ah[s] = p[s];
}

// ---- query staging ---------------------------------------------------------------------------------------------------------
// ntq query tiles from row qc0 of the query whose first row is qrow0 -> bq; rows >= nq stage as zero (score_split_q's rule)
// fp32 Q split on the fly: [tile][hi | lo][32][MT_BROW]
__device__ __forceinline__ void mt_stage_q_f32(_Float16* bq, const float* Qf, size_t qrow0, int qc0, int ntq, int nq, int tid) {
    for (int e = tid; e < ntq * 512; e += 256) {
        const int piece = e & 15, row = (e >> 4) & 31, qt = e >> 9, r = qc0 + qt * 32 + row;
        f16x8 hi8, lo8;
        if (r < nq) {
            mt_split8(reinterpret_cast<const float4*>(Qf + (qrow0 + r) * FLMR_DIM + piece * 8), hi8, lo8);
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) { hi8[k] = (_Float16)0.0f; lo8[k] = (_Float16)0.0f; }
        }
        *reinterpret_cast<f16x8*>(bq + ((qt * 2 + 0) * 32 + row) * MT_BROW + piece * 8) = hi8;
        *reinterpret_cast<f16x8*>(bq + ((qt * 2 + 1) * 32 + row) * MT_BROW + piece * 8) = lo8;
    }
}
// fp16 Q as it is, the hi plane only: [tile][32][MT_BROW]
__device__ __forceinline__ void mt_stage_q_f16(_Float16* bq, const _Float16* Qh, size_t qrow0, int qc0, int ntq, int nq, int tid) {
    for (int e = tid; e < ntq * 512; e += 256) {
        const int piece = e & 15, row = (e >> 4) & 31, qt = e >> 9, r = qc0 + qt * 32 + row;
        f16x8 hi8;
        if (r < nq) {
            hi8 = *reinterpret_cast<const f16x8*>(Qh + (qrow0 + r) * FLMR_DIM + piece * 8);
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) hi8[k] = (_Float16)0.0f;
        }
        *reinterpret_cast<f16x8*>(bq + (qt * 32 + row) * MT_BROW + piece * 8) = hi8;
    }
}

// ---- one 32 x 32 tile ------------------------------------------------------------------------------------------------------
// token of accumulator register r of a lane in half-wave h, tile t (the C/D layout of the 32x32 MFMA).  The loop that collects a
// lane's `okbits` from it stays written out in each kernel: as a shared function it cost the padded kernel registers (163 / 188
// VGPRs against 160 / 173 on this toolchain).
__device__ __forceinline__ int mt_row(int t, int r, int h) { return t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h; }

// The products of document tile (ah, al) with staged query tile qt.  hi(D) x hi(Q) always; QLO: hi(D) x lo(Q) (Q is fp32: PL = 2
// planes staged); DLO: lo(D) x hi(Q) (the document row has a low part; else `al` is not read).  An accumulator whose product is
// not issued stays the +0.0f the full kernel accumulates from all-zero low parts.
template <bool QLO, bool DLO>
__device__ __forceinline__ void mt_products(const _Float16* bq, int qt, int i, int h, const f16x8 (&ah)[8], const f16x8 (&al)[8],
                                            f32x16& acch, f32x16& accl, f32x16& accm) {
    constexpr int PL = QLO ? 2 : 1;
#pragma unroll
    for (int r = 0; r < 16; r++) { acch[r] = 0.0f; accl[r] = 0.0f; accm[r] = 0.0f; }
#pragma unroll
    for (int s = 0; s < 8; s++) {
        const f16x8 bh = *reinterpret_cast<const f16x8*>(bq + ((qt * PL + 0) * 32 + i) * MT_BROW + 64 * h + 8 * s);
        f16x8 bl;
        if constexpr (QLO) bl = *reinterpret_cast<const f16x8*>(bq + ((qt * PL + 1) * 32 + i) * MT_BROW + 64 * h + 8 * s);
        acch = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s], bh, acch, 0, 0, 0);
        if constexpr (QLO) accl = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s], bl, accl, 0, 0, 0);
        if constexpr (DLO) accm = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[s], bh, accm, 0, 0, 0);
    }
}

// ---- the LDS column state ----------------------------------------------------------------------------------------------------
// plain: the order-preserving uint image of the fp32 column maximum.  ARGMAX: the 64-bit key f2ord(v) << 32 | ~token, whose high
// word is that image and whose low word makes ties go to the LOWEST token, as torch's max(dim) does under autograd.  0 is below
// every real value in both.
template <bool ARGMAX>
using mt_col_t = std::conditional_t<ARGMAX, unsigned long long, unsigned int>;
__device__ __forceinline__ unsigned long long mt_key(float v, int token) {
    return ((unsigned long long)flmr_f2ord(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)token);
}
__device__ __forceinline__ float mt_col_value(unsigned long long key) { return flmr_ord2f((unsigned int)(key >> 32)); }
__device__ __forceinline__ float mt_col_value(unsigned int ord) { return flmr_ord2f(ord); }
__device__ __forceinline__ int mt_key_token(unsigned long long key) { return (int)(0xFFFFFFFFu - (uint32_t)key); }

// Fold of one tile's accumulators into column `col` (= the query row this lane's i names): the combine with the -9999 rule, the
// lane's maximum over its 16 rows (ARGMAX: with the lowest row holding it -- rows ascend with r for a fixed h), the half-wave
// exchange with the tie rule, one LDS atomic per column from half-wave 0.
template <bool ARGMAX>
__device__ __forceinline__ void mt_fold(const f32x16& acch, const f32x16& accl, const f32x16& accm, uint32_t okbits, int t, int h, int Ld,
                                        int col, int nq, mt_col_t<ARGMAX>* cols) {
    float mx = FLMR_NEG_INF;
    int arg = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = mt_row(t, r, h);
        const float v = ((okbits >> r) & 1u) ? fmaf(accl[r] + accm[r], 1.0f / 2048.0f, acch[r]) : -9999.0f;  // colbert.py:240
        if constexpr (ARGMAX) {
            if (row < Ld && v > mx) { mx = v; arg = row; }
        } else {
            if (row < Ld) mx = fmaxf(mx, v);
        }
    }
    if constexpr (ARGMAX) {
        const float omx = __shfl_xor(mx, 32, 64);
        const int oarg = __shfl_xor(arg, 32, 64);
        if (omx > mx || (omx == mx && oarg < arg)) { mx = omx; arg = oarg; }
        if (h == 0 && col < nq && mx > FLMR_NEG_INF) atomicMax(&cols[col], mt_key(mx, arg));
    } else {
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        if (h == 0 && col < nq && mx > FLMR_NEG_INF) atomicMax(&cols[col], flmr_f2ord(mx));
    }
}

// The epilogue, after the barrier that ends the tile walk: argmax (ARGMAX), the column maxima, their sequential ascending-column
// sum by thread 0.  has_cols: this document has column values (else -inf / -1); ok(token): the winner is a real token (else -1),
// a lambda that captures by VALUE (by reference it cost colbert_score_padded_mfma_kernel<true> its 173rd-VGPR limit).
template <bool ARGMAX, class OK>
__device__ __forceinline__ void mt_epilogue(const mt_col_t<ARGMAX>* cols, bool has_cols, OK ok, size_t ob, int nq, int tid,
                                            float* out, float* colmax_out, int32_t* argmax_out) {
    auto cmax = [&](int k) -> float { return has_cols ? mt_col_value(cols[k]) : FLMR_NEG_INF; };
    if constexpr (ARGMAX)
        for (int k = tid; k < nq; k += 256) {
            const int tok = has_cols ? mt_key_token(cols[k]) : -1;
            argmax_out[ob * nq + k] = (tok >= 0 && ok(tok)) ? tok : -1;
        }
    if (colmax_out)
        for (int k = tid; k < nq; k += 256) colmax_out[ob * nq + k] = cmax(k);
    if (tid == 0 && out) {
        float sc = 0.0f;
        for (int k = 0; k < nq; k++) sc += cmax(k);
        out[ob] = sc;
    }
}
