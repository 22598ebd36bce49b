// Internal helpers shared by the HIP translation units of libflmr_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "flmr_hip.h"

#define FLMR_DIM 128            // embedding width this build is specialised for
#define FLMR_WAVE 64            // CDNA wavefront
#define FLMR_MAX_NCELLS 8
#define FLMR_MAX_NQ_CAND 128    // candidate-generation width limit (4 column tiles of 32)
#define FLMR_MAX_NDOCS 8192
#define FLMR_SORTED_MAX_DOCLEN 2048   // longest passage of an index that gets a sorted code copy (sort_doc_codes_kernel sorts a passage in LDS)
// ints readable behind the sorted code copy, all of them code 0.  The dense stage 1 requests a later chunk of a round's codes for
// EVERY candidate of the round once one of them has that many: a 1-token passage that closes the index, in a round with a passage
// of FLMR_SORTED_MAX_DOCLEN codes, is read less than FLMR_SORTED_MAX_DOCLEN + 256 (the largest chunk) ints behind its start
// (flmr_stage1_dense.hip derives the bound next to its static_assert); the stage-2 walk reads 8 ints behind a run
#define FLMR_CODE_PAD (FLMR_SORTED_MAX_DOCLEN + 256)

extern thread_local char flmr_err_buf[512];

#define FLMR_FAIL(code, ...)                                     \
    do {                                                         \
        snprintf(flmr_err_buf, sizeof(flmr_err_buf), __VA_ARGS__); \
        return (code);                                           \
    } while (0)

#define FLMR_HIP(expr)                                                                              \
    do {                                                                                            \
        hipError_t e__ = (expr);                                                                    \
        if (e__ != hipSuccess) {                                                                    \
            snprintf(flmr_err_buf, sizeof(flmr_err_buf), "%s:%d: %s -> %s", __FILE__, __LINE__, #expr, \
                     hipGetErrorString(e__));                                                       \
            return FLMR_ERR_HIP;                                                                    \
        }                                                                                           \
    } while (0)

#define FLMR_LAUNCH_CHECK() FLMR_HIP(hipGetLastError())

// ---- variant switches (A/B runs, cross-check tests) ------------------------------------------------------------------
// The FLMR_* environment variables are read and parsed ONCE per process (first use of the library); afterwards the switches
// change only through flmr_set_option(), which accepts exactly the values below.  A searcher snapshots them when it is created
// and plans every batch from that snapshot (flmr_plan, flmr_search.hip): nothing on the per-batch launch path calls getenv, and
// no launcher reads a switch -- each receives the kernel form chosen for it.
enum class s0_sw : uint8_t { dflt, qs1, f16, f16rs, f32, valu };    // FLMR_S0_IMPL (mfma = f32)
enum class s1_sw : uint8_t { dflt, scan, slots, image };            // FLMR_S1_IMPL
enum class s2_sw : uint8_t { dflt, xcda, xcd, walk, lds, regs, ldsb };   // FLMR_S2_IMPL (regs / ldsb: FLMR_EXPERIMENTAL_VARIANTS builds)
enum class s3_sw : uint8_t { dflt, qs, lean, cw, cwregs, dma, regs, f32 };   // FLMR_S3_IMPL
struct flmr_options {
    s0_sw s0;                 // unset: fp16-split, query-stationary + "hi first" on the sparse path | qs1 ("hi first" with the dense epilogue
                              // inside the loop) | f16 (both products everywhere) | f16rs (row-stationary fp16 kernel) | f32 / mfma | valu
    s1_sw s1;                 // scan: code-scanning stage 1 for every query | slots: the slot form of the scatter kernel for every query
                              // (default: its queue form first) | image: the queries beyond the dense images go to the scan
    s2_sw s2;                 // xcda (approximate-then-refine on the sliced kernel: the default where the sliced kernel is) | xcd | walk |
                              // lds (the LDS-DMA gather) | regs / ldsb (measured losers) -- default: cost model
    s3_sw s3;                 // lean (default for Nq <= 32) | cw | cwregs | dma | regs (the register maxsim_f16_kernel) | qs (query-stationary
                              // kernel for long queries) | f32 (fp32-MFMA kernel)
    bool full_table;          // FLMR_FULL_TABLE: keep the whole centroid-score table
    bool cand_atomic;         // FLMR_CAND_IMPL=atomic: first candidate-generation implementation
    bool cand_bitmaps;        // FLMR_CAND_IMPL=bitmaps: the queue form marks the probed cells' candidate bitmap for every query (it skips it
                              // by default where every surviving centroid is a probed cell: flmr_cand_args::implied)
    bool s1_no_hitmap;        // FLMR_S1_NO_HITMAP: no hit prefilter
    bool s0_staged;           // FLMR_S0_STAGED: staged epilogue for every tile
    bool s3_no_multiq;        // FLMR_S3_NO_MULTIQ: single-tile MaxSim kernel for long queries too
    bool score_valu;          // FLMR_SCORE_IMPL=valu: plain-FMA padded scorer
    bool poison;              // FLMR_POISON (test runs): every batch and every phase 1 starts with EVERY scratch buffer of the searcher's
                              // workspace refilled over its whole allocation (the record kept by ws_alloc, flmr_search.hip): floats, halves
                              // and 64-bit keys with 0xFF bytes, counts / offsets / ids / masks with 0 -- a stage that lives off an earlier
                              // batch's workspace then produces NaNs or loses its survivors; only the deferred status words are carried
    int32_t row_cap;          // FLMR_ROW_CAP: score rows a searcher keeps per query (64 .. 65535; 0 = the default 16384, at most K): a query
                              // with more centroids above the threshold has its stage 1 recomputed
};
// the process switches; FLMR_ERR_INVALID (naming the variable) while the environment holds a value the library does not know
int flmr_process_options(flmr_options* out);

static inline int64_t flmr_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int64_t flmr_round_up(int64_t a, int64_t b) { return flmr_ceil_div(a, b) * b; }

// Workgroups per query (grid.y) of the kernels whose waves each take every W-th document of a query (W = waves in the grid row):
// enough to put `target_waves` waves on the chip, but never more than 64 documents per wave -- the kernels keep a wave's documents
// one per lane, this is the launch contract their "<= 64" comments name -- nor fewer than one document per workgroup, and >= 1.
static inline int flmr_doc_grid(int target_waves, int waves_per_workgroup, int nqueries, int max_count) {
    int G = (int)flmr_ceil_div(target_waves, waves_per_workgroup * (int64_t)nqueries);
    const int gmin = (int)flmr_ceil_div(max_count, waves_per_workgroup * 64);
    const int gmax = (int)flmr_ceil_div(max_count, waves_per_workgroup);
    if (G < gmin) G = gmin;
    if (G > gmax) G = gmax;
    return G < 1 ? 1 : G;
}

// ---- the argument rules of the MaxSim entry points (padded, typed, gathered, index; forward and backward) -------------------
// One statement of each rule, INVALID before UNSUPPORTED.  An entry point keeps only what is its own (NULL pointers, dtypes,
// which sizes it has, where an empty batch returns) and switches a rule off by passing the value that satisfies it:
//   q_batch, B, cross   the padded forms' query rule: q_batch is 1 or B; the cross form takes 1..65535 queries (a grid dimension).
//                       Off: 1, 1, 0
//   sizes_ok            the entry point's own sizes are in range.  Off: true
//   ptrs                OR of the pointers whose rows are read 16 bytes at a time.  Off: 0
//   dim                 the build's embedding width.  Off: FLMR_DIM
//   nq, nq_max          the query columns whose state the kernel keeps in LDS.  Off: FLMR_MAXSIM_NQ_ANY
#define FLMR_MAXSIM_NQ_KEYS ((size_t)64 * 1024 / 8)   // 8-byte (value, ~token) keys in 64 KiB
#define FLMR_MAXSIM_NQ_ANY (~(size_t)0)
static inline int flmr_maxsim_check(int32_t q_batch, int32_t B, int32_t cross, bool sizes_ok, uintptr_t ptrs, int32_t dim, int32_t nq,
                                    size_t nq_max) {
    if (!cross && q_batch != 1 && q_batch != B) FLMR_FAIL(FLMR_ERR_INVALID, "q_batch must be 1 or B");
    if (cross && (q_batch < 1 || q_batch > 65535)) FLMR_FAIL(FLMR_ERR_INVALID, "cross scoring takes 1..65535 queries per call");
    if (!sizes_ok) FLMR_FAIL(FLMR_ERR_INVALID, "bad sizes");
    if (ptrs & 15) FLMR_FAIL(FLMR_ERR_INVALID, "the query, document and gradient rows must be 16-byte aligned");
    if (dim != FLMR_DIM) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "dim=%d (this build: %d)", dim, FLMR_DIM);
    if ((size_t)nq > nq_max) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "nq=%d too large", nq);
    return FLMR_OK;
}

// ---- (score, pid) keys -----------------------------------------------------------------------
// The reference selects with std::priority_queue<std::pair<float,int>> (filter_pids.cpp:24): descending
// lexicographic (score, pid).  A 64-bit key whose unsigned order equals that order lets one integer
// compare / radix pass do the same: high word = order-preserving map of the fp32 score, low word = pid.
__host__ __device__ static inline uint32_t flmr_f2ord(float f) {
    if (f == 0.0f) f = 0.0f;  // -0.0 == +0.0 for the reference's float compare
    uint32_t u;
    memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ static inline float flmr_ord2f(uint32_t o) {
    uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
__host__ __device__ static inline uint64_t flmr_make_key(float score, int32_t pid) {
    return ((uint64_t)flmr_f2ord(score) << 32) | (uint32_t)pid;
}
__host__ __device__ static inline int32_t flmr_key_pid(uint64_t key) { return (int32_t)(uint32_t)key; }
__host__ __device__ static inline float flmr_key_score(uint64_t key) { return flmr_ord2f((uint32_t)(key >> 32)); }

// ---- index object ----------------------------------------------------------------------------
struct flmr_index {
    int32_t dim, nbits, K, device;
    int64_t N, num_passages, pid_base;
    int32_t packed_dim;  // dim*nbits/8 bytes per token
    bool owns;           // arrays below were hipMalloc'ed by flmr_index_open
    int32_t* codes;
    uint8_t* residuals;
    int64_t* doc_offsets;
    int32_t* ivf_pids;
    int64_t* ivf_offsets;
    float* centroids;
    float* wlut;  // [256][8/nbits] fused decode table: bucket_weights[lut[rev[byte]][l]]
    _Float16* centroids_f16;  // [K,128] fp16 image of the centroids (only when centroids_f16_exact)
    uint32_t* wtab16;   // fp16 hi / lo images of wlut as MFMA A-operand fragments per residual byte (S3 "cw" form; flmr_maxsim.hip)
    float* inv_norm;    // [N + 64] 1 / max(||centroid + weights||, 1e-12) per token (S3 "cw" form); NULL when unavailable
    float bucket_weights[256];
    // host copy of the IVF list lengths sorted descending, prefix-summed: bound on #candidates for c cells
    int64_t* ivf_len_prefix;  // [K+1] host
    int64_t max_doclen;
    int32_t centroids_f16_exact;  // every centroid value is representable in fp16 (true for reference-format indexes)
    uint32_t* ivf_chunk_tab;      // [K][nchunks+1]: first entry of each IVF list with pid >= chunk*32768
    int32_t nchunks;
    int32_t* codes_sorted;        // [N + FLMR_CODE_PAD] per-passage ascending copy of `codes` with the DISTINCT values first (the rest of a
                                  // passage's run repeats its largest code: still ascending, the same set), the pad filled with code 0; NULL when a passage
                                  // is longer than FLMR_SORTED_MAX_DOCLEN
    uint16_t* doc_ulen;           // [num_passages] distinct codes per passage = the length of the distinct prefix in codes_sorted; NULL when
                                  // fewer than a tenth of the tokens repeat a code of their passage (every token then counts)
    double dup_share;             // share of the tokens that repeat a code of their passage (0 when codes_sorted was not built)
    double mean_ulen;             // mean number of distinct codes per passage
    _Float16* centroids_f16_tiled;  // centroids_f16 in MFMA A-operand order, one contiguous 1 KB run per (tile, k-step) (stage-2 walk)
    uint16_t* doc_splits;         // [num_passages][nslices]: codes_sorted position of the first code >= s * slice_rows (XCD-sliced stage 2)
    float cen_norm_max;           // >= the largest centroid 2-norm (bound of the "hi first" stage 0)
    int32_t nslices;              // 8, 16, 24 or 32: the fp16 centroid table cut so that a slice fits an XCD's L2
    int32_t slice_rows;           // ceil(K / nslices)
    int32_t xcd_round_robin;      // probed at open: workgroup L of a 1-D grid runs on XCD (L % 8) of 8
};
int flmr_build_sorted_codes(flmr_index* ix);
int flmr_build_tiled_centroids(flmr_index* ix, bool forced);   // forced: FLMR_S2_IMPL=walk
int flmr_build_doc_splits(flmr_index* ix);
int flmr_build_s3_tables(flmr_index* ix);   // wtab16 + inv_norm (optional: left NULL when they cannot be built)

// build the fused byte -> (8/nbits) fp32 decode table from the codec tables (host)
void flmr_build_wlut(int nbits, const float* bucket_weights, const uint8_t* reversed_bit_map,
                     const uint8_t* combos, float* wlut /* [256 * 8/nbits] */);
void flmr_default_codec_tables(int nbits, uint8_t* reversed_bit_map /*256*/, uint8_t* combos /*256*8/nbits*/);

// ---- kernels' host launchers (defined in the stage .hip files) ---------------------------------
struct flmr_s0_args {
    const float* centroids;  // [K,128]
    const float* Q;          // [nqueries, nq, 128]
    const int32_t* q_lens;   // nullable
    int32_t K, nqueries, nq, nq_cand, ncol, ncells;
    float thr;
    float* cs;               // [nqueries, K, ncol]
    uint32_t* idx_bits;      // [nqueries, idx_words]
    int32_t idx_words;
    float* part_val;         // [nqueries, nblk, ncol, ncells]
    int32_t* part_idx;
    int32_t nblk;            // number of partial-list row blocks (flmr_s0_choose: for the kernel it picks)
    int32_t* cells;          // [nqueries, max_cells]
    int32_t* ncell;          // [nqueries]
    int32_t max_cells;
    int32_t full_table;      // 1: store every row of the score table; 0: only rows of surviving centroids (fp16 S0, nq_cand<=32)
    const _Float16* centroids_f16;  // [K,128] (nullable)
    int32_t part_rows;       // 0: partials are per-block top-ncells lists; >0: partials are per-block column MAXIMA over
                             // `part_rows` centroid rows and s0_select_cells rescans the winning blocks in the table
    _Float16* q_hi;          // [nqueries, ncol, 128] fp16 split of Q (fp16 MFMA path)
    _Float16* q_lo;          //   Q ~= q_hi + q_lo * 2^-11
    int32_t centroids_f16_exact;
    int32_t q_hi_only;       // FLMR_NUMERICS_GPU_FP16: Q is ROUNDED to fp16 (q_lo = 0), as the reference's `Q.cuda().half()`
    // "hi first" stage 0 (sparse query-stationary path): the hi products alone give every score to within q_err[query][column];
    // the lo products are computed only for the tiles that can hold a surviving row, the block maxima stay hi-only and
    // s0_select_cells verifies its choice against that bound (flmr_stage0.hip).  q_err == NULL: both products everywhere.
    float* q_err;            // [nqueries, ncol] rigorous bound on |c . q_lo| / 2048 (+ the combine's rounding), written by s0_prepare_kernel
    float* q_err_buf;        // where s0_prepare_kernel writes (the sparse query-stationary path always fills it: stage 2's
                             // approximate-then-refine form reads it too); q_err == q_err_buf when stage 0 itself uses the bound
    float* q_err_sum;        // [nqueries] bound on |approximate - full| for a passage's stage-2 score (sum over the columns + summation rounding)
    float cen_norm_max;      // >= max_c ||c||_2
    int32_t grp_blocks;      // flmr_s0_choose: > 0 = the kernel it picked ALSO leaves one column maximum per `grp_blocks`
                             // consecutive 64-row blocks, as floats [nqueries, nblk / grp_blocks, ncol] in the part_idx buffer (unused on
                             // that path): s0_select_cells reads those first and only the best groups' block maxima after them
};
// stage-0 kernel forms: query-stationary (qs2: "hi first" / fp16 numerics; qs), row-stationary fp16 (sparse table / whole table), fp32
// MFMA, plain FMA
enum class s0_form : uint8_t { qs2, qs, f16_sparse, f16_table, f32, valu };
struct flmr_s0_choice {
    s0_form form;
    int32_t nblk, part_rows, grp_blocks;   // the partial-list geometry of that form (flmr_s0_args fields of the same names)
};
flmr_s0_choice flmr_s0_choose(const flmr_s0_args& a, const flmr_options& o);
int flmr_launch_centroid_scores(const flmr_s0_args& a, s0_form form, hipStream_t st);
int flmr_launch_select_cells(const flmr_s0_args& a, hipStream_t st);
int flmr_launch_centroid_argmax(flmr_s0_args a, int32_t* out_codes, hipStream_t st);  // index build: nearest centroid per column
int flmr_launch_split_q(const flmr_s0_args& a, hipStream_t st);  // q_hi / q_lo images only (query-split stage 0)
int flmr_check_f16_exact(const float* dev, size_t n, int32_t* host_result);
int flmr_convert_f16(const float* dev, size_t n, _Float16* out);
int flmr_max_row_norm(const float* dev, int64_t rows, float* host_result);   // >= max_r ||row_r||_2 over [rows, 128] (rounded up)

int flmr_launch_ivf_mark(const int32_t* cells, const int32_t* ncell, int32_t max_cells, int32_t nqueries,
                         const int32_t* ivf_pids, const int64_t* ivf_offsets, uint32_t* bitmap, int64_t bitmap_words,
                         hipStream_t st);
int flmr_launch_compact(const uint32_t* bitmap, int64_t bitmap_words, int64_t num_passages, int32_t nqueries,
                        int32_t* cand, int64_t cand_cap, int32_t* cand_count, int32_t* overflow, hipStream_t st);

struct flmr_filter_args {
    const float* cs;           // score rows: the full table [nqueries, K, ncol] (row = centroid id, stride K*ncol), or -- cs_compact --
                               // only the rows of each query's surviving centroids, [nqueries, row_cap, ncol], row = RANK of the
                               // centroid among the set bits of the query's idx mask (written by qualifying_kernel)
    int64_t cs_query_stride;
    int32_t cs_compact;
    int32_t row_cap;            // compact form: rows per query (a rank beyond it -- a query over capacity, flagged by qualifying_kernel -- is clamped)
    const uint32_t* idx_prefix; // [nqueries, idx_words] exclusive popcount of the idx words before each word (compact rows' ranks)
    int32_t K, ncol, nq_cand, nqueries;
    const int32_t* q_lens;     // nullable (effective columns = min(q_len, nq_cand))
    const int32_t* codes;
    const int64_t* doclens;    // nullable -> offsets[p+1]-offsets[p]
    const int64_t* offsets;
    int32_t f16_round;         // FLMR_NUMERICS_GPU_FP16: column maxima rounded to fp16, fp32 sum rounded to fp16 (flmr_device.h)
    const uint16_t* ulen_sorted;  // nullable: distinct codes per passage -- the part of a passage's run in `codes_sorted` the sliced stage 2
                                  // reads (a maximum is idempotent: filter_pids.cpp:50-63)
};
// stage 1: candidates (cand[q*cand_stride + i], i < cand_count[q]) restricted to idx_bits -> keys
int flmr_launch_filter_stage1(const flmr_filter_args& f, const uint32_t* idx_bits, int32_t idx_words,
                              const int32_t* cand, int64_t cand_stride, const int32_t* cand_count, uint64_t* keys,
                              const uint32_t* hit_bits, int64_t hit_words, const int32_t* hit_valid,
                              const uint8_t* hit_flags, hipStream_t st, const int32_t* skip = nullptr);
// chunked candidate generation (flmr_candidates.hip): bitmaps in LDS per (query, 32768-passage chunk)
#define FLMR_FAST_HDR 0
struct flmr_cand_args {
    int32_t nqueries, idx_words, max_cells, qmax, nchunks;
    int64_t words, cand_cap;
    const uint32_t* idx_bits; const int32_t* cells; const int32_t* ncell;
    const int32_t* ivf_pids; const int64_t* ivf_offsets; const uint32_t* chunk_tab;
    int32_t* qual; int32_t* nqual; int32_t* hit_valid;     // [nqueries, qmax], [nqueries], [nqueries]
    uint32_t* cand_bits; uint32_t* hit_bits; int32_t* chunk_cnt;  // [nqueries, words] x2, [nqueries, nchunks]
    int32_t* cand; uint8_t* cand_hit; int32_t* cand_count; int32_t* overflow;
    // stage 1 by scatter over the surviving centroids' IVF lists (cand_mark_score_kernel), for queries with hit_valid
    int32_t scatter;                 // 0: bitmaps only (stage 1 = filter_stage1_kernel for every query)
    const float* cs; int64_t cs_query_stride; int32_t nq_cand; const int32_t* q_lens;
    // compact score rows (flmr_filter_args::cs_compact): qualifying_kernel computes them -- rows_out [nqueries, qmax, 32], row j =
    // the j-th surviving centroid's scores, the stage-0 MFMA sequence on the fp16 centroid rows (bitwise the values stage 0
    // computes) -- and `cs` points at the same buffer; rows_out == NULL: `cs` is the full table written by stage 0
    float* rows_out; const _Float16* cen16; const _Float16* q_hi; const _Float16* q_lo; uint32_t* idx_prefix;
    int32_t cs_compact;
    uint64_t* keys; int32_t* key_count;   // [nqueries, cand_cap] unordered stage-1 keys, [nqueries] running count
    int32_t* chunk_hits;                  // [nqueries, nchunks] candidates of the chunk that are in the hit set (scatter mode)
    int32_t n_select;                     // how many keys the selection after stage 1 keeps (ndocs)
    int32_t f16_round;                    // see flmr_filter_args
    // the queue and small-dense forms of the scatter kernel and their hand-over to the slot form: per query of the batch [b] the plan
    // word written by cand_plan_kernel from statistics measured on a sample of the query's chunks (0 queue form, FLMR_PLAN_SMALL
    // small-dense form, 1 slot form), overwritten by the forms with what happened (FLMR_TAP_STAGE1_FORM: 2 / 4 = handed over to the slot
    // form after the queue / small-dense form ran into a limit, 3 = done by the small-dense form), and [B + b] the fast forms' own key
    // counter.  Nothing in it outlives the batch.  NULL: slot kernel only (FLMR_S1_IMPL=slots)
    int32_t* fast_state;
    // which queries the dense stage-1 forms take (flmr_launch_s1_dense_modes' outputs), written by cand_plan_kernel when it runs -- one
    // launch less per batch; s1d_mode == NULL: not fused
    int32_t* s1d_mode; int32_t* s1d_scan_skip; int32_t* s1d_any; int32_t s1d_img_rows, s1d_exact_too;
    int32_t* row_ovf;   // [nqueries] out: 1 = the query has more surviving centroids than compact score rows (qmax): its stage 1 is
                        // recomputed from the fp16 centroids (flmr_launch_filter_stage1_recompute); NULL on the full-table path
    // "cells imply candidates", per query [b], written by cand_plan_kernel: 1 = the query is non-empty, hit_valid holds and every
    // surviving centroid is one of its probed cells, so every passage of a surviving list is a candidate by that same list.  The queue
    // form then neither loads the probed cells' lists nor writes cand_bits / chunk_cnt for the query: nothing in the search reads them
    // unless the query ends with fewer than n_select hit candidates, and then cand_mark_score_kernel (which knows the final count) marks
    // them from `cells` before cand_emit_kernel appends the other candidates.  Readers outside the search (FLMR_TAP_CANDIDATES) get
    // them from flmr_launch_cand_emit_all, which marks them first for the queries that went without (flmr_cand_bitmaps_state == 1):
    // for that, cells / ncell, implied, fast_state, hit_bits and chunk_hits of the last batch stay untouched until the next batch or
    // phase 1 starts.  NULL (or force_bitmaps, FLMR_CAND_IMPL=bitmaps): the cells are marked for every query.
    int32_t* implied; int32_t force_bitmaps;
};
// what became of query b's candidate bitmap on the list-scatter path (flmr_searcher_cand_bitmaps): 0 = marked in the scatter pass (flag
// clear, or another form than the queue form finished the query), 1 = never needed inside the search (skipped), 2 = skipped in the
// pass and marked afterwards inside the search (fewer than n_select hit candidates)
__host__ __device__ static inline int flmr_cand_bitmaps_state(int implied, int plan_word, int key_count, int n_select) {
    if (!implied || plan_word != 0) return 0;
    return key_count >= n_select ? 1 : 2;
}
int flmr_launch_candidates_chunked(const flmr_cand_args& a, hipStream_t st);
int flmr_launch_qualifying(const flmr_cand_args& a, hipStream_t st);   // list + ranks + compact score rows only
int flmr_launch_cand_emit_all(const flmr_cand_args& a, hipStream_t st);   // (marks the candidate bitmaps a flagged query went without first)
int flmr_build_chunk_table(const int32_t* ivf_pids, const int64_t* ivf_offsets, int K, int64_t num_passages,
                           uint32_t** out_tab, int32_t* out_nchunks);
// passage bitmap of the union of the surviving centroids' IVF lists (+ per-query validity flag)
int flmr_launch_hit_bitmap(const uint32_t* idx_bits, int32_t idx_words, int32_t nqueries, const int32_t* ivf_pids,
                           const int64_t* ivf_offsets, const int32_t* cand_count, uint32_t* hit_bits, int64_t hit_words,
                           int32_t* hit_valid, hipStream_t st);
// stage 2: all centroids, one wave per document
int flmr_launch_filter_stage2(const flmr_filter_args& f, const int32_t* pids, int64_t pid_stride,
                              const int32_t* counts, int32_t max_count, uint64_t* keys, int64_t key_stride,
                              hipStream_t st);
// stage 2 without the score table: recompute the survivors' centroid scores from the fp16 centroids (bitwise = S0)
// (form: lds = the LDS-DMA gather; regs / ldsb = the measured losers of FLMR_EXPERIMENTAL_VARIANTS builds)
int flmr_launch_filter_stage2_mfma(const flmr_filter_args& f, const int32_t* pids, int64_t pid_stride, const int32_t* counts,
                                   int32_t max_count, uint64_t* keys, int64_t key_stride, const _Float16* cen16,
                                   const _Float16* q_hi, const _Float16* q_lo, s2_sw form, hipStream_t st);
// stage 2 as a query-stationary dense walk over the centroid table (flmr_stage2_walk.hip): same keys, bit for bit
int flmr_launch_filter_stage2_walk(const flmr_filter_args& f, const int32_t* pids, int64_t pid_stride, const int32_t* counts,
                                   int32_t max_count, uint64_t* keys, int64_t key_stride, const _Float16* cen16,
                                   const _Float16* q_hi, const _Float16* q_lo, const int32_t* codes_sorted, hipStream_t st);
bool flmr_stage2_walk_pays(const flmr_index* ix, int nqueries, int max_count);
// stage 1 of the queries flagged in row_ovf (more surviving centroids than compact score rows) recomputed from the fp16 centroids
int flmr_launch_filter_stage1_recompute(const flmr_filter_args& f, const uint32_t* idx_bits, int32_t idx_words, const int32_t* cand,
                                        int64_t cand_stride, const int32_t* cand_count, const int32_t* row_ovf, uint64_t* keys,
                                        const _Float16* cen16, const _Float16* q_hi, const _Float16* q_lo, hipStream_t st);
// stage 2 with the centroid table cut into one L2-resident slice per XCD (flmr_stage2_xcd.hip): same keys, bit for bit;
// `part`: workspace of flmr_stage2_xcd_part_floats(max_queries, part_stride) floats
int flmr_launch_filter_stage2_xcd(const flmr_filter_args& f, const int32_t* pids, int64_t pid_stride, const int32_t* counts,
                                  int32_t max_count, uint64_t* keys, int64_t key_stride, const flmr_index* ix,
                                  const _Float16* q_hi, const _Float16* q_lo, float* part, int64_t part_stride, hipStream_t st);
bool flmr_stage2_xcd_pays(const flmr_index* ix);
size_t flmr_stage2_xcd_part_floats(const flmr_index* ix, int64_t nqueries, int64_t ndocs);
// hi_only: the hi products alone (the fp16 numerics mode, where they ARE the scores; or the approximate pass of the
// approximate-then-refine form below)
int flmr_launch_filter_stage2_xcd_ex(const flmr_filter_args& f, const int32_t* pids, int64_t pid_stride, const int32_t* counts,
                                     int32_t max_count, uint64_t* keys, int64_t key_stride, const flmr_index* ix,
                                     const _Float16* q_hi, const _Float16* q_lo, float* part, int64_t part_stride, bool hi_only,
                                     hipStream_t st);
// Stage-2 survivor selection from APPROXIMATE keys (hi-only scores, each within err_sum[q] of the full one): the passages
// certainly inside the top n go straight to out_pids, the passages within 2 err of the cut form the band whose full scores
// decide the rest (flmr_launch_s2_refine_finish after the band has been rescored).
int flmr_launch_s2_refine_plan(const uint64_t* keys, int64_t key_stride, const int32_t* counts, int32_t max_count, int32_t nqueries,
                               int32_t n, const float* err_sum, int32_t* out_pids, int64_t out_stride, int32_t* band_pids,
                               int64_t band_stride, int32_t* band_count, int32_t* need, int32_t* def_count, hipStream_t st);
int flmr_launch_s2_refine_finish(const uint64_t* band_keys, int64_t key_stride, const int32_t* band_count, const int32_t* need,
                                 const int32_t* def_count, int32_t max_count, int32_t nqueries, int32_t* out_pids,
                                 int64_t out_stride, int32_t* n_out, hipStream_t st);
// top-n of count[q] keys, unordered output (radix select); n_out[q] = min(n, count[q])
int flmr_launch_select_topn(const uint64_t* keys, int64_t key_stride, const int32_t* counts, int32_t nqueries,
                            int32_t n, int32_t* out_pids, int64_t out_stride, int32_t* n_out, hipStream_t st,
                            uint64_t* out_keys = nullptr, uint64_t key_add = 0);
// exact sharded protocol helpers (keys carry GLOBAL pids between ranks; 0 = empty)
int flmr_launch_select_keys(const uint64_t* keys, int32_t nqueries, int32_t m, int32_t n, uint64_t* out, hipStream_t st);
int flmr_launch_sort_keys_topn(const uint64_t* keys, int32_t nqueries, int32_t m, int32_t n, uint64_t* out,
                               int32_t* out_counts, hipStream_t st);
int flmr_launch_filter_local_keys(const uint64_t* keys, int32_t nqueries, int32_t n_in, int64_t pid_base,
                                  int64_t num_passages, int32_t* out_pids, int64_t out_stride, int32_t* out_count,
                                  hipStream_t st, int32_t* out_slot = nullptr);
int flmr_launch_export_keys_slotted(const uint64_t* keys, int64_t key_stride, const int32_t* counts, const int32_t* slot,
                                    int32_t nqueries, uint64_t key_add, int32_t n, uint64_t* out, hipStream_t st);
int flmr_launch_export_keys(const uint64_t* keys, int64_t key_stride, const int32_t* counts, int32_t nqueries, uint64_t key_add,
                            int32_t n, uint64_t* out, hipStream_t st);
int flmr_launch_unpack_keys(const uint64_t* keys, int32_t nqueries, int32_t n, int32_t k, int32_t* out_pids, float* out_scores,
                            int32_t* out_counts, hipStream_t st);
// sorted (descending key) top-n of count[q] <= FLMR_MAX_NDOCS keys; writes pids (+ optional scores), n_out.
// pad_pid / pad_score fill positions [n_out, n) when fill != 0.
int flmr_launch_sort_topn(const uint64_t* keys, int64_t key_stride, const int32_t* counts, int32_t max_count,
                          int32_t nqueries, int32_t n, int32_t* out_pids, float* out_scores, int64_t out_stride,
                          int32_t* n_out, int64_t pid_base, int fill, hipStream_t st);

struct flmr_maxsim_args {
    const flmr_index* ix;
    const float* Q;           // [nqueries, nq, 128]
    const int32_t* q_lens;    // nullable
    int32_t nqueries, nq;
    const int32_t* pids;      // [nqueries, pid_stride]
    int64_t pid_stride;
    const int32_t* counts;    // [nqueries]
    int32_t max_count;
    uint64_t* keys;           // out [nqueries, key_stride] (score,pid) keys   (nullable)
    int64_t key_stride;
    float* scores;            // out [nqueries, key_stride] fp32 scores        (nullable)
    _Float16* q_hi;           // scratch [nqueries, round_up(nq,32), 128]: fp16 split of Q (nullable -> fp32 MFMA kernel)
    _Float16* q_lo;
    int32_t gpu_fp16;         // FLMR_NUMERICS_GPU_FP16: the reference's CUDA-path scoring (fp16 embeddings, -9999 padding, no clamp)
    int32_t q_split_done;     // 1: q_hi / q_lo already hold this batch's images (stage 0 made the same ones: nq <= 32 <= nq_cand)
    // workspace of the planned-tile kernels (nullable -> the kernels that walk the passages themselves):
    uint2* plan_desc;         // [nqueries, plan_stride] one descriptor per 32-token tile of a query's finalists
    int64_t plan_stride;      // >= max_count * ceil(max_doclen / 32)
    int32_t* plan_wbeg;       // [nqueries, plan_wcap] first tile of every wave's share (+ the end)
    int32_t plan_wcap;        // >= waves per query + 1
    float* colmax_ws;         // long queries: [nqueries, key_stride, round_up(nq, 32)] per-passage column maxima (nullable)
    int64_t colmax_cap;       // floats
};
// stage-3 kernel forms (flmr_maxsim.hip): query-stationary on planned tiles (long queries), multi-tile, planned tiles ("lean"),
// centroid + weight on the LDS-DMA pipeline, the same with register gathers, LDS-DMA decompress, register decompress
// (maxsim_f16_kernel), fp32 MFMA; the fp16-numerics pipeline / its plain form
enum class s3_form : uint8_t { qs, multiq, lean, cw, cwregs, dma, regs, f32, gpu_tuned, gpu_plain };
s3_form flmr_s3_choose(const flmr_maxsim_args& a, const flmr_options& o);
int flmr_launch_maxsim(const flmr_maxsim_args& a, s3_form form, hipStream_t st);

// ---- stage 1 for dense survivor sets (flmr_stage1_dense.hip) ----
struct flmr_s1d_args {
    const int32_t* codes;        // `codes_sorted`: per-passage runs, distinct values first, FLMR_CODE_PAD ints of code 0 behind the last
    const int64_t* offsets;      // [num_passages + 1]
    const uint16_t* ulen;        // [num_passages] distinct codes per passage (NULL: every token, offsets[p+1] - offsets[p])
    const uint32_t* idx_bits;    // [nqueries, idx_words] surviving-centroid mask (index_storage.py:116)
    const uint32_t* idx_prefix;  // [nqueries, idx_words] exclusive popcount per word (qualifying_kernel)
    int32_t idx_words;
    const float* rows;           // compact score rows [nqueries, row_cap, 32] (row = rank of the centroid among the survivors)
    int32_t row_cap;
    const int32_t* nqual;        // [nqueries] surviving centroids (clamped to row_cap by qualifying_kernel)
    const int32_t* q_lens;       // nullable
    int32_t nq_cand, nqueries;
    const int32_t* cand;         // [nqueries, cand_stride] ascending candidate pids
    int64_t cand_stride;
    const int32_t* cand_count;
    const int32_t* band;         // [nqueries, cand_stride] the band of an image query (EXACT pass)
    const int32_t* band_count;
    const int32_t* mode;         // [nqueries] FLMR_S1D_*: which queries this launch takes, from which list
    uint64_t* keys;              // [nqueries, cand_stride] out
    float* img_err;              // [nqueries] out (IMG pass): E + eps of the band rule (inf: the images cannot be used)
    int32_t parts;               // items per query (0: the launcher's choice)
    int32_t group;               // candidates per wave and group: 64, or 16 for short lists
    int64_t codes_len;           // tokens at `codes`; FLMR_CODE_PAD more ints, each a valid code, must be readable behind them (every chunk of a round)
    int32_t img_rows;            // rows of images the launch's LDS holds (IMG pass; set by the launcher)
    const int32_t* any;          // nullable: [0] some query takes the IMG pass, [1] some query takes the EXACT pass (flmr_launch_s1_dense_modes)
};
#define FLMR_S1D_SKIP 0    // stage 1 of the query is done elsewhere (list-scatter forms, the round-5 scan)
#define FLMR_S1D_IMAGE 1   // IMG pass over the candidates, band, EXACT pass over the band
#define FLMR_S1D_EXACT 2   // EXACT pass over the candidates
// `mean_codes` = the index's mean number of (distinct) codes per passage: 16 or 32 lanes per candidate x 4 or 8 codes per lane
int flmr_s1_dense_image_rows(int nqueries, int idx_words, double mean_codes);   // score-row images the LDS form holds per query (0: K too large)
int flmr_launch_s1_image(const flmr_s1d_args& a, double mean_codes, hipStream_t st);   // the approximate pass (U keys, img_err)
int flmr_launch_s1_exact(const flmr_s1d_args& a, double mean_codes, hipStream_t st);   // the exact pass (bands, whole lists)
// which queries the dense forms take: mode[q] = SKIP where skip[q] (done by a list-scatter form) or row_ovf[q] (no rows: the
// recompute form), IMAGE where the query's rows fit
// `img_rows` images, else EXACT (exact_too) or SKIP with scan[q] = 0 (the round-5 scan takes the query); scan[q] = 1 everywhere else
int flmr_launch_s1_dense_modes(const int32_t* skip, const int32_t* nqual, const int32_t* row_ovf, int32_t nqueries, int32_t img_rows,
                               int32_t exact_too, int32_t* mode, int32_t* scan_skip, int32_t* any, hipStream_t st);
// the band of every IMAGE query from its U keys (keys >= the n-th largest - err[q]) -> band pids / counts; in_count[q] = the number
// of keys the top-n selection after stage 1 reads for query q (band_count for IMAGE queries, counts[q] for the others)
int flmr_launch_s1_band(const uint64_t* keys, int64_t key_stride, const int32_t* counts, const int32_t* mode, const float* err,
                        int32_t nqueries, int32_t n, int32_t* band, int32_t* band_count, int32_t* in_count, hipStream_t st);

int flmr_launch_exclusive_scan_lengths(const int32_t* pids, const int64_t* doclens, const int64_t* offsets, int32_t n,
                                       int64_t* out_offsets /* [n+1] */, hipStream_t st);
