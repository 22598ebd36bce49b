// Retrieve-and-rescore for RAG training (src/models/rag/rag_model_blip.py:409-442): the GATHERED forms of the padded MaxSim
// under autograd, flmr_maxsim_gather_fwd / _bwd.
//
// Output row r = q * k + j scores query q against passage pids[q, j] of a device-resident store [npassages, Ld, 128] (fp32 or
// fp16) with mask [npassages, Ld].  The forward runs the tile body of flmr_maxsim_tile.h -- the one
// colbert_score_padded_mfma_kernel<true> (flmr_ops.hip) runs: staging of Q, tile walk, accumulation, (value, ~token) LDS key --
// with the document base taken from the pid and the query block from r / k, so out / colmax / argmax are bit-identical to
// flmr_colbert_maxsim_fwd on Q.repeat_interleave(k) and store[pids] -- neither of which is ever built.  An fp16 store value has
// a zero low part, so the third product of the split (lo(D) x hi(Q)) is identically +0 and is not issued: two MFMAs per 16 dims
// instead of three and half the bytes per token row, with the same bits as the fp32 kernel gives the widened values.
// The backward writes dQ alone (the store is a constant of training): one wave per (q, i), the k rows of the query walked in
// ascending j -- a fixed order, no floating-point atomics.
//
// flmr_maxsim_index_fwd / _bwd are the same two kernels with a third source of document rows: the resident compressed index
// (flmr_index).  Where a token row comes from is the kernels' compile-time parameter, a LOADER: the fp32 store, the fp16 store,
// or the index at nbits 1 / 2 / 4 / 8, whose loader decodes a lane's half row (code -> centroid half-row, 8 * nbits residual
// bytes -> bucket weights), normalises it and splits it into the fp16 hi / lo operand.  Passage p's tokens are
// doc_offsets[p] .. doc_offsets[p + 1]: no mask array, no common padded length, no uncompressed copy of the corpus.
#include "flmr_maxsim_tile.h"

typedef _Float16 rh2 __attribute__((ext_vector_type(2)));

// ---- document-row loaders -------------------------------------------------------------------------------------------
// What the two kernels ask of a loader L (passed by value as a kernel argument):
//   L::LO                     the fp16 split of a row has a low part: the third product (lo(D) x hi(Q)) is issued
//   L::lds_bytes()            dynamic LDS of its own behind the kernel's (a decode table), staged by stage()
//   doc open(pid)             the passage of this workgroup: live (there are tokens to walk), len (tokens walked),
//                             cols (an all-padded document still has column values: -9999 held by token 0)
//   ok(doc, row)              token `row` (< len) is a real, unmasked token
//   load(doc, tok, h, ah, al) dims 64 h .. 64 h + 63 of token `tok` as hi / lo MFMA A fragments (tokens >= len re-read token 0);
//                             called by whole waves
//   row2(pid, a, lane, d)     backward: dims 2 lane, 2 lane + 1 of token a of passage pid; false = nothing to add (wave-uniform)
struct rs_doc {
    bool live, cols;
    int len;
    size_t base;            // store: the passage's first row; index: its first token
    const uint8_t* mrow;    // store: the passage's mask row
};

template <bool F16>
struct rs_store_loader {
    static constexpr bool LO = !F16;
    const void* store;
    const uint8_t* store_mask;
    int npassages, Ld;
    __host__ __device__ static constexpr size_t lds_bytes() { return 0; }
    __device__ __forceinline__ void stage(char*, int) const {}
    __device__ __forceinline__ rs_doc open(int pid) const {
        rs_doc d;
        // an empty slot is an all-padded document: every token scores -9999, nothing is read (a pid past the store, the caller's
        // error, is kept from reading out of bounds the same way)
        d.live = pid >= 0 && pid < npassages;
        d.cols = Ld > 0;
        d.len = Ld;
        d.base = (size_t)pid * Ld;
        d.mrow = store_mask + (size_t)(d.live ? pid : 0) * Ld;
        return d;
    }
    __device__ __forceinline__ bool ok(const rs_doc& d, int row) const { return d.mrow[row] != 0; }
    __device__ __forceinline__ void load(const rs_doc& d, const char*, int tok, int h, f16x8 (&ah)[8], f16x8 (&al)[8]) const {
        const size_t drow = (d.base + (tok < Ld ? tok : 0)) * FLMR_DIM + 64 * h;   // (rows past Ld re-read token 0)
        if constexpr (F16) mt_load_row_f16(reinterpret_cast<const _Float16*>(store) + drow, ah);
        else mt_load_row_f32(reinterpret_cast<const float*>(store) + drow, ah, al);
    }
    __device__ __forceinline__ bool row2(int p, int a, int lane, float2& d) const {
        if (a < 0 || a >= Ld || p < 0 || p >= npassages) return false;
        const size_t off = ((size_t)p * Ld + a) * FLMR_DIM + 2 * lane;
        if constexpr (F16) {
            const rh2 hv = *reinterpret_cast<const rh2*>(reinterpret_cast<const _Float16*>(store) + off);
            d = make_float2((float)hv[0], (float)hv[1]);
        } else {
            d = *reinterpret_cast<const float2*>(reinterpret_cast<const float*>(store) + off);
        }
        return true;
    }
};

// The compressed index as the document source.  Token t of passage p is row x / max(||x||, 1e-12) with x = centroids[codes[t]] +
// the bucket weights of its residual bytes (decompress_residuals.cpp:69-71, then F.normalize: index_storage.py:160-173), all in
// fp32 from the fp32 centroid table -- an index whose centroids are not fp16-representable has no fp16 image and no inv_norm
// table, so neither is used.  The norm is reduced in the kernel: 64 squares per lane in ascending dim, the two halves added.
// The byte -> weights table (flmr_index::wlut, 256 x 8 / nbits floats: 8 KB at nbits 1 .. 1 KB at nbits 8) is staged in LDS and
// read with one vector read per byte.
template <int NBITS>
struct rs_index_loader {
    static constexpr bool LO = true;
    static constexpr int VPB = 8 / NBITS;             // dims per residual byte
    static constexpr int PACKED = FLMR_DIM / VPB;     // residual bytes per token
    const int32_t* codes;
    const uint8_t* residuals;
    const int64_t* doc_offsets;
    const float* centroids;
    const float* wlut;
    int64_t num_passages, pid_base;
    int K;
    __host__ __device__ static constexpr size_t lds_bytes() { return (size_t)256 * VPB * sizeof(float); }
    __device__ __forceinline__ void stage(char* lds, int tid) const {
        float* t = reinterpret_cast<float*>(lds);
        for (int e = tid; e < 256 * VPB; e += 256) t[e] = wlut[e];
    }
    __device__ __forceinline__ rs_doc open(int pid) const {
        rs_doc d;
        // pids are the searcher's (global): local = pid - pid_base.  An empty slot, a pid outside the index and a passage of
        // length 0 are all-padded documents: every column -9999, argmax -1, nothing read
        const int64_t p = (int64_t)pid - pid_base;
        const bool in = pid >= 0 && p >= 0 && p < num_passages;
        const int64_t off = in ? doc_offsets[p] : 0;
        d.len = in ? (int)(doc_offsets[p + 1] - off) : 0;
        d.live = d.len > 0;
        d.cols = true;
        d.base = (size_t)off;
        d.mrow = nullptr;
        return d;
    }
    __device__ __forceinline__ bool ok(const rs_doc&, int) const { return true; }
    __device__ __forceinline__ int code_of(size_t tc) const {
        const int c = codes[tc];
        return (unsigned)c < (unsigned)K ? c : 0;   // (a corrupt code must not read past the centroid table)
    }
    __device__ __forceinline__ void weights(const float* tab, uint32_t byte, float (&w)[VPB]) const {
        if constexpr (VPB == 8) {
            const float4 x = reinterpret_cast<const float4*>(tab)[byte * 2], y = reinterpret_cast<const float4*>(tab)[byte * 2 + 1];
            w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w; w[4] = y.x; w[5] = y.y; w[6] = y.z; w[7] = y.w;
        } else if constexpr (VPB == 4) {
            const float4 x = reinterpret_cast<const float4*>(tab)[byte];
            w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
        } else if constexpr (VPB == 2) {
            const float2 x = reinterpret_cast<const float2*>(tab)[byte];
            w[0] = x.x; w[1] = x.y;
        } else {
            w[0] = tab[byte];
        }
    }
    __device__ __forceinline__ void load(const rs_doc& d, const char* lds, int tok, int h, f16x8 (&ah)[8], f16x8 (&al)[8]) const {
        const float* tab = reinterpret_cast<const float*>(lds);
        const size_t tc = d.base + (tok < d.len ? tok : 0);   // (rows past the passage end re-read token 0)
        const float4* c4 = reinterpret_cast<const float4*>(centroids + (size_t)code_of(tc) * FLMR_DIM + 64 * h);
        const uint2* r2 = reinterpret_cast<const uint2*>(residuals + tc * PACKED + h * (PACKED / 2));
        float x[64];
#pragma unroll
        for (int t = 0; t < 16; t++) {
            const float4 v = c4[t];
            x[4 * t + 0] = v.x; x[4 * t + 1] = v.y; x[4 * t + 2] = v.z; x[4 * t + 3] = v.w;
        }
        float ss = 0.0f;
#pragma unroll
        for (int wq = 0; wq < NBITS; wq++) {
            const uint2 pk = r2[wq];
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const uint32_t byte = ((e < 4 ? pk.x : pk.y) >> (8 * (e & 3))) & 255u;
                float w[VPB];
                weights(tab, byte, w);
#pragma unroll
                for (int l = 0; l < VPB; l++) {
                    const int dd = (wq * 8 + e) * VPB + l;
                    x[dd] = w[l] + x[dd];               // `weight + centroid`, decompress_residuals.cpp:69-71
                    ss = fmaf(x[dd], x[dd], ss);
                }
            }
        }
        ss += __shfl_xor(ss, 32, 64);
        float nrm = sqrtf(ss);
        nrm = nrm < 1e-12f ? 1e-12f : nrm;
        const float inv = 1.0f / nrm;
#pragma unroll
        for (int s = 0; s < 8; s++) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] = x[8 * s + e] * inv;
            mt_split8(v, ah[s], al[s]);
        }
    }
    // the winner row decoded on the fly: the lane's two dims share a residual byte (two bytes at nbits 8); the norm is the wave's
    // sum of the 64 lanes' squares by a fixed butterfly
    __device__ __forceinline__ bool row2(int pid, int a, int lane, float2& d) const {
        const int64_t p = (int64_t)pid - pid_base;
        if (a < 0 || pid < 0 || p < 0 || p >= num_passages) return false;
        const int64_t off = doc_offsets[p];
        if (a >= doc_offsets[p + 1] - off) return false;
        const size_t tc = (size_t)off + a;
        const float2 c = *reinterpret_cast<const float2*>(centroids + (size_t)code_of(tc) * FLMR_DIM + 2 * lane);
        float w0, w1;
        if constexpr (VPB == 1) {
            const uint32_t two = *reinterpret_cast<const uint16_t*>(residuals + tc * PACKED + 2 * lane);
            w0 = wlut[two & 255u];
            w1 = wlut[two >> 8];
        } else {
            const uint32_t byte = residuals[tc * PACKED + (2 * lane) / VPB];
            w0 = wlut[byte * VPB + (2 * lane) % VPB];
            w1 = wlut[byte * VPB + (2 * lane) % VPB + 1];
        }
        const float x0 = w0 + c.x, x1 = w1 + c.y;
        float ss = fmaf(x1, x1, x0 * x0);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
        float nrm = sqrtf(ss);
        nrm = nrm < 1e-12f ? 1e-12f : nrm;
        const float inv = 1.0f / nrm;
        d = make_float2(x0 * inv, x1 * inv);
        return true;
    }
};

// The ARGMAX tile body of flmr_maxsim_tile.h with the document taken from loader L by pid and the query block from row / k.
template <class L>
__global__ __launch_bounds__(256, 2) void maxsim_gather_fwd_kernel(const float* __restrict__ Qf, int nq, int nqp, const L ld,
                                                                   const int32_t* __restrict__ pids, int k,
                                                                   float* out, float* colmax_out, int32_t* argmax_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const mt_lds<2, unsigned long long> Y{nqp, L::lds_bytes()};
    _Float16* bq = reinterpret_cast<_Float16*>(smem + Y.bq);
    unsigned long long* colkey = reinterpret_cast<unsigned long long*>(smem + Y.cols);   // [nqp] (value, ~token)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, h = lane >> 5;
    const size_t ob = blockIdx.x;
    const size_t qrow0 = (ob / (size_t)k) * nq;
    const char* ltab = smem + Y.ltab;   // the loader's own LDS
    const rs_doc doc = ld.open(pids[ob]);
    const bool live = doc.live;
    const int Ld = doc.len;
    if (live) ld.stage(const_cast<char*>(ltab), tid);   // (ordered before the first tile by the barriers of the first pass)
    // what the tile walk leaves in a column of an all-padded document: -9999 held by token 0
    const unsigned long long padkey = mt_key(-9999.0f, 0);
    for (int c = tid; c < nqp; c += 256) colkey[c] = (!live && doc.cols && c < nq) ? padkey : 0ull;
    const int ntiles = live ? (Ld + 31) >> 5 : 0;
    for (int qc0 = 0; qc0 < nq && live; qc0 += 32 * MT_QC) {
        const int ntq = mt_chunk_tiles(nq, qc0);
        __syncthreads();
        mt_stage_q_f32(bq, Qf, qrow0, qc0, ntq, nq, tid);   // fp32 Q split on the fly
        __syncthreads();
        for (int t = wave; t < ntiles; t += 4) {
            const int tok = t * 32 + i;
            f16x8 ah[8], al[8];
            ld.load(doc, ltab, tok, h, ah, al);
            uint32_t okbits = 0;   // which of this lane's 16 accumulator rows are real, unmasked tokens (bit r)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = mt_row(t, r, h);
                if (row < Ld && ld.ok(doc, row)) okbits |= 1u << r;
            }
            for (int qt = 0; qt < ntq; qt++) {
                f32x16 acch, accl, accm;
                mt_products<true, L::LO>(bq, qt, i, h, ah, al, acch, accl, accm);   // fp16 store: no lo(D) x hi(Q)
                mt_fold<true>(acch, accl, accm, okbits, t, h, Ld, qc0 + qt * 32 + i, nq, colkey);
            }
        }
    }
    __syncthreads();
    mt_epilogue<true>(colkey, doc.cols, [=](int tok) { return live && ld.ok(doc, tok); }, ob, nq, tid, out, colmax_out, argmax_out);
}

// one wave per (query q, column i); lane l owns dims 2l, 2l+1; the k rows of the query 64 at a time, added in ascending j
template <class L>
__global__ __launch_bounds__(256) void maxsim_gather_grad_q_kernel(const L ld,
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
            float2 d;
            if (!ld.row2(p, a, lane, d)) continue;
            acc.x = fmaf(g, d.x, acc.x);
            acc.y = fmaf(g, d.y, acc.y);
        }
    }
    *reinterpret_cast<float2*>(dQ + (size_t)pair * FLMR_DIM + 2 * lane) = acc;
}

static int gather_sizes(int32_t store_dtype, int32_t npassages, int32_t Ld, int32_t dim, int32_t nqueries, int32_t k, int32_t nq) {
    if (store_dtype != FLMR_F32 && store_dtype != FLMR_F16) FLMR_FAIL(FLMR_ERR_INVALID, "store_dtype=%d (FLMR_F32 or FLMR_F16)", store_dtype);
    const int rc = flmr_maxsim_check(1, 1, 0, nq >= 1 && nqueries >= 0 && k >= 0 && npassages >= 0 && Ld >= 0, 0, dim, nq, FLMR_MAXSIM_NQ_KEYS);
    if (rc) return rc;
    if ((int64_t)nqueries * k > 0x7fffffffll) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "nqueries * k = %lld rows", (long long)nqueries * k);
    return FLMR_OK;
}

template <class L>
static int launch_fwd(const L& ld, const float* Q, int32_t nqueries, int32_t nq, const int32_t* pids, int32_t k, float* out, float* colmax,
                      int32_t* argmax, hipStream_t st) {
    const int nqp = (int)((nq + 31) / 32 * 32);
    const size_t lds = mt_lds<2, unsigned long long>{nqp, L::lds_bytes()}.bytes;
    const dim3 grid((unsigned)((int64_t)nqueries * k));
    FLMR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(maxsim_gather_fwd_kernel<L>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(maxsim_gather_fwd_kernel<L>, grid, dim3(256), lds, st, Q, (int)nq, nqp, ld, pids, (int)k, out, colmax, argmax);
    FLMR_LAUNCH_CHECK();
    return FLMR_OK;
}

template <class L>
static int launch_bwd(const L& ld, const int32_t* pids, int32_t nqueries, int32_t k, int32_t nq, const int32_t* argmax, const float* G,
                      float* dQ, hipStream_t st) {
    const int64_t pairs = (int64_t)nqueries * nq;
    const dim3 grid((unsigned)flmr_ceil_div(pairs, 4));
    hipLaunchKernelGGL(maxsim_gather_grad_q_kernel<L>, grid, dim3(256), 0, st, ld, pids, (int)nqueries, (int)k, (int)nq, argmax, G, dQ);
    FLMR_LAUNCH_CHECK();
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
    const int ra = flmr_maxsim_check(1, 1, 0, true, reinterpret_cast<uintptr_t>(store) | reinterpret_cast<uintptr_t>(Q), FLMR_DIM, nq, FLMR_MAXSIM_NQ_ANY);
    if (ra) return ra;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (store_dtype == FLMR_F16)
        return launch_fwd(rs_store_loader<true>{store, store_mask, (int)npassages, (int)Ld}, Q, nqueries, nq, pids, k, out, colmax, argmax, st);
    return launch_fwd(rs_store_loader<false>{store, store_mask, (int)npassages, (int)Ld}, Q, nqueries, nq, pids, k, out, colmax, argmax, st);
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
    if (store_dtype == FLMR_F16)
        return launch_bwd(rs_store_loader<true>{store, nullptr, (int)npassages, (int)Ld}, pids, nqueries, k, nq, argmax, grad_colmax, dQ, st);
    return launch_bwd(rs_store_loader<false>{store, nullptr, (int)npassages, (int)Ld}, pids, nqueries, k, nq, argmax, grad_colmax, dQ, st);
}

// ---- the compressed index as the store ------------------------------------------------------------------------------
static int index_sizes(const flmr_index* ix, int32_t nqueries, int32_t k, int32_t nq) {
    if (!ix) FLMR_FAIL(FLMR_ERR_INVALID, "NULL index");
    const int rc = flmr_maxsim_check(1, 1, 0, nq >= 1 && nqueries >= 0 && k >= 0, 0, ix->dim, nq, FLMR_MAXSIM_NQ_KEYS);
    if (rc) return rc;
    if (ix->nbits != 1 && ix->nbits != 2 && ix->nbits != 4 && ix->nbits != 8) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "nbits=%d", ix->nbits);
    if ((int64_t)nqueries * k > 0x7fffffffll) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "nqueries * k = %lld rows", (long long)nqueries * k);
    return FLMR_OK;
}

template <int NBITS>
static rs_index_loader<NBITS> index_loader(const flmr_index* ix) {
    return rs_index_loader<NBITS>{ix->codes, ix->residuals, ix->doc_offsets, ix->centroids, ix->wlut, ix->num_passages, ix->pid_base, (int)ix->K};
}
#define RS_NB(call)                                  \
    switch (ix->nbits) {                             \
        case 1: return call(index_loader<1>(ix));    \
        case 2: return call(index_loader<2>(ix));    \
        case 4: return call(index_loader<4>(ix));    \
        default: return call(index_loader<8>(ix));   \
    }

extern "C" int flmr_maxsim_index_fwd(const flmr_index_t* ix, const float* Q, int32_t nqueries, int32_t nq, const int32_t* pids, int32_t k,
                                     float* out, float* colmax, int32_t* argmax, flmr_stream_t stream) {
    const int rc = index_sizes(ix, nqueries, k, nq);
    if (rc) return rc;
    if ((int64_t)nqueries * k == 0) return FLMR_OK;
    if (!Q || !pids || !argmax) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    const int ra = flmr_maxsim_check(1, 1, 0, true, reinterpret_cast<uintptr_t>(Q), FLMR_DIM, nq, FLMR_MAXSIM_NQ_ANY);
    if (ra) return ra;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define RS_FWD(ld) [&](const auto& l) { return launch_fwd(l, Q, nqueries, nq, pids, k, out, colmax, argmax, st); }(ld)
    RS_NB(RS_FWD)
#undef RS_FWD
}

extern "C" int flmr_maxsim_index_bwd(const flmr_index_t* ix, const int32_t* pids, int32_t nqueries, int32_t k, int32_t nq,
                                     const int32_t* argmax, const float* grad_colmax, float* dQ, flmr_stream_t stream) {
    const int rc = index_sizes(ix, nqueries, k, nq);
    if (rc) return rc;
    if ((int64_t)nqueries * k == 0) return FLMR_OK;   // (nothing is launched: dQ is the caller's to zero)
    if (!dQ || !pids || !argmax || !grad_colmax) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define RS_BWD(ld) [&](const auto& l) { return launch_bwd(l, pids, nqueries, k, nq, argmax, grad_colmax, dQ, st); }(ld)
    RS_NB(RS_BWD)
#undef RS_BWD
}
