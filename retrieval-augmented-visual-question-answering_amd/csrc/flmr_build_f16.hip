// Fused fp16 compress (flmr_compress_f16): nearest centroid + residual bucketize + bit-pack in ONE pass over fp16 token rows,
// what ResidualCodec.compress does on the GPU (colbert/indexing/codecs/residual.py:169-204, which rounds the batch to half
// before its `centroids @ batch.T` argmax).
//
// Shape (token-stationary, one pass, no partials in global memory):
//   - a 512-thread workgroup owns T = 512 tokens: 8 waves x 64 tokens, each wave's tokens held for the whole launch as the B
//     operands of v_mfma_f32_32x32x16_f16 (two 32-token column blocks x 8 k-steps = 64 VGPRs per lane);
//   - the fp16 centroid table streams through LDS in 64-row tiles (16 KB, double-buffered: the next tile's global loads are in
//     flight while the current one is multiplied; one barrier per tile; rows padded to 272 B so the A-operand reads of a
//     half-wave hit 16 distinct 4-bank groups);
//   - fp16 x fp16 products are exact in fp32, so ONE MFMA product per score (the fp32 path, flmr_nearest_centroids, splits
//     every row into hi + lo and runs two);
//   - every lane keeps a running (max, index) for its token over the 16 accumulator rows it owns, scanned in ascending centroid
//     order with a strict '>' (the lowest index wins a tie inside the lane); at the end the two half-waves holding the same
//     token merge lexicographically (larger score, then lower index);
//   - epilogue in the same workgroup: the winning centroid row is gathered, the residual float(e) - float(c) is formed from
//     the token row still in registers, bucketized against the cut-offs (torch.bucketize, right=False) and packed in the
//     reference's bit order -- the same bytes flmr_compress_residuals writes for emb.float().
// The whole table is read once per workgroup: K x 256 B, i.e. 64 KB of L2 / MALL traffic per token at K = 2^17 against
// 2 x 128 x K flop (512 flop per byte).
//
// fp16 subnormals.  Whether the f16 MFMA keeps subnormal A / B inputs is a property of the hardware mode we do not want the
// codes to depend on (a dot-product instruction was found to flush them).  So no subnormal ever reaches the MFMA: every token
// row is multiplied by 2^s_t (its largest magnitude lands in [2^14, 2^15)) and the centroid table by one common 2^s_c (same
// rule over the whole table).  Multiplying an fp16 value by a power of two that keeps it below 2^16 is exact, products of
// fp16 values are exact in fp32, so every score is the unscaled fp32 score times 2^(s_t + s_c): the argmax over c is the
// same, subnormal components included, whether or not the MFMA would have flushed them.  (The shift lifts every subnormal
// to a normal number for rows / tables whose largest magnitude is below 32; unit rows -- what encoders emit -- get 14.)
// The residual epilogue undoes the row scale exactly and reads the winning centroid from the caller's table.
#include <hip/hip_runtime.h>

#include "flmr_common.h"
#include "flmr_device.h"

namespace {

constexpr int CF_WAVES = 8;                  // waves per workgroup
constexpr int CF_THREADS = CF_WAVES * 64;
constexpr int CF_TOK = CF_WAVES * 64;        // tokens per workgroup (T)
constexpr int CF_CT = 64;                    // centroid rows per LDS tile
constexpr int CF_ROWB = FLMR_DIM * 2 + 16;   // LDS bytes per centroid row (256 + 16 B pad)
constexpr int CF_TILE_CHUNKS = CF_CT * FLMR_DIM * 2 / 16;   // 16-byte pieces per tile (1024)
static_assert(CF_TILE_CHUNKS % CF_THREADS == 0, "tile load split");
constexpr int CF_LOADS = CF_TILE_CHUNKS / CF_THREADS;       // per thread per tile (2)

// largest |x| of the table as fp16 bits (non-negative halves order like unsigned integers)
__global__ __launch_bounds__(256) void f16_absmax_kernel(const uint16_t* __restrict__ src, size_t count,
                                                          uint32_t* __restrict__ out) {
    uint32_t m = 0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (size_t)gridDim.x * blockDim.x) {
        const uint32_t a = src[e] & 0x7fffu;
        m = a > m ? a : m;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t v = (uint32_t)__shfl_xor((int)m, o, 64);
        m = v > m ? v : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// the power-of-two shift that brings a largest magnitude m (fp16 bits) into [2^14, 2^15); 0 for m >= 2^14 or m == 0
__device__ __forceinline__ int f16_shift_for(uint32_t m_bits) {
    if (m_bits == 0) return 0;
    const float m = (float)__builtin_bit_cast(_Float16, (uint16_t)m_bits);
    const int s = 14 - ilogbf(m);
    return s > 0 ? s : 0;
}

// dst [Kpad, 128] = src * 2^s_c, rows K..Kpad-1 := row 0 (an exact duplicate can never win the first-index argmax)
__global__ __launch_bounds__(256) void f16_scale_pad_kernel(const uint16_t* __restrict__ src, int64_t K, int64_t Kpad,
                                                             const uint32_t* __restrict__ absmax, _Float16* __restrict__ dst) {
    const float scale = ldexpf(1.0f, f16_shift_for(*absmax));
    const size_t total = (size_t)Kpad * FLMR_DIM;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t row = e / FLMR_DIM;
        const uint16_t b = row < (size_t)K ? src[e] : src[e % FLMR_DIM];
        dst[e] = (_Float16)((float)__builtin_bit_cast(_Float16, b) * scale);
    }
}

template <int NBITS>
__global__ __launch_bounds__(CF_THREADS) void compress_f16_kernel(const _Float16* __restrict__ cen_scaled, int64_t Kpad,
                                                                  const _Float16* __restrict__ cen, const _Float16* __restrict__ emb,
                                                                  int64_t n, const float* __restrict__ cutoffs,
                                                                  int32_t* __restrict__ out_codes, uint8_t* __restrict__ out) {
    constexpr int NCUT = (1 << NBITS) - 1, VPB = 8 / NBITS;
    constexpr int LANE_BYTES = 64 / VPB;     // a lane packs 64 dims = 8 * NBITS bytes
    __shared__ __attribute__((aligned(16))) uint8_t tile[2][CF_CT * CF_ROWB];
    __shared__ float cut[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, h = lane >> 5;
    for (int t = tid; t < 256; t += CF_THREADS) cut[t] = t < NCUT ? cutoffs[t] : __builtin_inff();

    // ---- the wave's 64 tokens: lane (i, h) holds dims [64h, 64h + 64) of tokens tok0 + i and tok0 + 32 + i ----
    const int64_t tok0 = (int64_t)blockIdx.x * CF_TOK + wave * 64;
    f16x8 b[2][8];
    int shift[2];
#pragma unroll
    for (int bb = 0; bb < 2; bb++) {
        const int64_t tok = tok0 + bb * 32 + i;
        const f16x8* p = reinterpret_cast<const f16x8*>(emb + tok * FLMR_DIM + 64 * h);
        float m = 0.0f;
#pragma unroll
        for (int s = 0; s < 8; s++) {
            if (tok < n) b[bb][s] = p[s];
            else {
#pragma unroll
                for (int j = 0; j < 8; j++) b[bb][s][j] = (_Float16)0.0f;
            }
#pragma unroll
            for (int j = 0; j < 8; j++) m = fmaxf(m, fabsf((float)b[bb][s][j]));
        }
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        shift[bb] = f16_shift_for(__builtin_bit_cast(uint16_t, (_Float16)m));
        const float scale = ldexpf(1.0f, shift[bb]);
#pragma unroll
        for (int s = 0; s < 8; s++)
#pragma unroll
            for (int j = 0; j < 8; j++) b[bb][s][j] = (_Float16)((float)b[bb][s][j] * scale);
    }

    // ---- stream the scaled centroid table through LDS ----
    const int64_t ntiles = Kpad / CF_CT;
    const uint4* gsrc = reinterpret_cast<const uint4*>(cen_scaled);
    uint4 pre[CF_LOADS];
    auto fetch = [&](int64_t t) {
#pragma unroll
        for (int j = 0; j < CF_LOADS; j++) pre[j] = gsrc[t * CF_TILE_CHUNKS + tid + j * CF_THREADS];
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int j = 0; j < CF_LOADS; j++) {
            const int q = tid + j * CF_THREADS;   // 16 pieces per row
            *reinterpret_cast<uint4*>(&tile[buf][(q >> 4) * CF_ROWB + (q & 15) * 16]) = pre[j];
        }
    };
    float best[2] = {-__builtin_inff(), -__builtin_inff()};
    int bidx[2] = {0, 0};
    fetch(0);
    stash(0);
    __syncthreads();
    for (int64_t t = 0; t < ntiles; t++) {
        const int buf = (int)(t & 1);
        if (t + 1 < ntiles) fetch(t + 1);
#pragma unroll
        for (int mb = 0; mb < 2; mb++) {
            f16x8 a[8];
            const uint8_t* row = &tile[buf][(mb * 32 + i) * CF_ROWB + 128 * h];
#pragma unroll
            for (int s = 0; s < 8; s++) a[s] = *reinterpret_cast<const f16x8*>(row + 16 * s);
            f32x16 acc0, acc1;
#pragma unroll
            for (int r = 0; r < 16; r++) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
#pragma unroll
            for (int s = 0; s < 8; s++) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s], b[0][s], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s], b[1][s], acc1, 0, 0, 0);
            }
            // accumulator r of lane (i, h) = centroid row (r & 3) + 8 (r >> 2) + 4h of the block: ascending in r
            const int base = (int)(t * CF_CT) + mb * 32 + 4 * h;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int c = base + (r & 3) + 8 * (r >> 2);
                if (acc0[r] > best[0]) { best[0] = acc0[r]; bidx[0] = c; }
                if (acc1[r] > best[1]) { best[1] = acc1[r]; bidx[1] = c; }
            }
        }
        if (t + 1 < ntiles) stash(buf ^ 1);
        __syncthreads();
    }

    // ---- merge the two half-waves, then the residual epilogue ----
#pragma unroll
    for (int bb = 0; bb < 2; bb++) {
        const float ob = __shfl_xor(best[bb], 32, 64);
        const int oi = __shfl_xor(bidx[bb], 32, 64);
        if (ob > best[bb] || (ob == best[bb] && oi < bidx[bb])) { best[bb] = ob; bidx[bb] = oi; }
        const int64_t tok = tok0 + bb * 32 + i;
        if (tok >= n) continue;
        const int code = bidx[bb];
        if (h == 0) out_codes[tok] = code;
        const float unscale = ldexpf(1.0f, -shift[bb]);
        const f16x8* pc = reinterpret_cast<const f16x8*>(cen + (size_t)code * FLMR_DIM + 64 * h);
        uint32_t words[LANE_BYTES / 4 > 0 ? LANE_BYTES / 4 : 1];
        uint32_t acc = 0;
#pragma unroll
        for (int s = 0; s < 8; s++) {
            const f16x8 c8 = pc[s];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int d = 8 * s + j;   // dim within the lane's 64
                const float r = (float)b[bb][s][j] * unscale - (float)c8[j];
                int bucket;
                if (NBITS <= 2) {
                    bucket = 0;
#pragma unroll
                    for (int k = 0; k < NCUT; k++) bucket += cut[k] < r ? 1 : 0;
                } else {
                    int lo = 0, hi = NCUT;   // first index whose cut-off is >= r
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (cut[mid] < r) lo = mid + 1; else hi = mid;
                    }
                    bucket = lo;
                }
                const uint32_t rev = __brev((uint32_t)bucket) >> (32 - NBITS);
                const int byte = d / VPB, l = d % VPB;
                acc |= (rev << (8 - NBITS * (l + 1))) << (8 * (byte & 3));
                if ((byte & 3) == 3 && l == VPB - 1) { words[byte >> 2] = acc; acc = 0; }
            }
        }
        uint32_t* dst = reinterpret_cast<uint32_t*>(out + (size_t)tok * (16 * NBITS) + (size_t)h * LANE_BYTES);
#pragma unroll
        for (int w = 0; w < LANE_BYTES / 4; w++) dst[w] = words[w];
    }
}

struct dev_buf {
    void* p = nullptr;
    ~dev_buf() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) {
        FLMR_HIP(hipMalloc(&p, bytes ? bytes : 1));
        return FLMR_OK;
    }
};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int flmr_compress_f16(const uint16_t* centroids_f16, int64_t K, const uint16_t* emb_f16, int64_t n,
                                 const float* bucket_cutoffs, int32_t nbits, int32_t* out_codes, uint8_t* out_residuals,
                                 flmr_stream_t stream) {
    if (!centroids_f16 || !emb_f16 || !bucket_cutoffs || !out_codes || !out_residuals) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    if (nbits != 1 && nbits != 2 && nbits != 4 && nbits != 8) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "nbits=%d (supported: 1, 2, 4, 8)", nbits);
    if (K < 1 || K > (1ll << 30) || n < 0) FLMR_FAIL(FLMR_ERR_INVALID, "bad sizes K=%lld n=%lld", (long long)K, (long long)n);
    if (!aligned16(centroids_f16) || !aligned16(emb_f16) || (reinterpret_cast<uintptr_t>(out_residuals) & 7))
        FLMR_FAIL(FLMR_ERR_INVALID, "centroids / emb must be 16-byte aligned, out_residuals 8-byte aligned");
    if (n == 0) return FLMR_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // workspace: the scaled, padded table + one word; independent of n
    const int64_t Kpad = flmr_round_up(K, CF_CT);
    dev_buf tab, mx;
    if (int rc = tab.alloc((size_t)Kpad * FLMR_DIM * sizeof(_Float16))) return rc;
    if (int rc = mx.alloc(sizeof(uint32_t))) return rc;
    FLMR_HIP(hipMemsetAsync(mx.p, 0, sizeof(uint32_t), st));
    const size_t count = (size_t)K * FLMR_DIM;
    const unsigned g1 = (unsigned)(count / 256 + 1 < 2048 ? count / 256 + 1 : 2048);
    hipLaunchKernelGGL(f16_absmax_kernel, dim3(g1), dim3(256), 0, st, centroids_f16, count, static_cast<uint32_t*>(mx.p));
    hipLaunchKernelGGL(f16_scale_pad_kernel, dim3(2048), dim3(256), 0, st, centroids_f16, K, Kpad,
                       static_cast<const uint32_t*>(mx.p), static_cast<_Float16*>(tab.p));
    FLMR_LAUNCH_CHECK();
    const int64_t blocks = (n + CF_TOK - 1) / CF_TOK;
    if (blocks > 0x7fffffffll) FLMR_FAIL(FLMR_ERR_INVALID, "n=%lld too large", (long long)n);
    const _Float16* ts = static_cast<const _Float16*>(tab.p);
    const _Float16* c16 = reinterpret_cast<const _Float16*>(centroids_f16);
    const _Float16* e16 = reinterpret_cast<const _Float16*>(emb_f16);
    switch (nbits) {
        case 1: hipLaunchKernelGGL(compress_f16_kernel<1>, dim3((unsigned)blocks), dim3(CF_THREADS), 0, st, ts, Kpad, c16, e16, n, bucket_cutoffs, out_codes, out_residuals); break;
        case 2: hipLaunchKernelGGL(compress_f16_kernel<2>, dim3((unsigned)blocks), dim3(CF_THREADS), 0, st, ts, Kpad, c16, e16, n, bucket_cutoffs, out_codes, out_residuals); break;
        case 4: hipLaunchKernelGGL(compress_f16_kernel<4>, dim3((unsigned)blocks), dim3(CF_THREADS), 0, st, ts, Kpad, c16, e16, n, bucket_cutoffs, out_codes, out_residuals); break;
        default: hipLaunchKernelGGL(compress_f16_kernel<8>, dim3((unsigned)blocks), dim3(CF_THREADS), 0, st, ts, Kpad, c16, e16, n, bucket_cutoffs, out_codes, out_residuals); break;
    }
    FLMR_LAUNCH_CHECK();
    FLMR_HIP(hipStreamSynchronize(st));  // the workspace is freed on return
    return FLMR_OK;
}
