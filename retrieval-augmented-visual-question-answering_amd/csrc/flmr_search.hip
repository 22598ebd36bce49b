// Batched search orchestration: workspace planning + the S0..S4 launch sequence on one HIP stream.
// Replaces Searcher._search_all_Q / dense_search / IndexScorer.rank (TPC/searcher.py:73-132,
// TPC/search/index_storage.py:67-182) for a whole batch of queries at once.
#include <new>

#include "flmr_common.h"

static const char* kStageNames[FLMR_NUM_STAGES] = {
    "s0_centroid_scores", "s0_select_cells", "s0_candidates", "s1_hitmap", "s1_filter", "s1_select", "s2_filter_sort",
    "s3_maxsim", "s4_topk"};

extern "C" const char* flmr_stage_name(int32_t s) { return (s >= 0 && s < FLMR_NUM_STAGES) ? kStageNames[s] : "?"; }

#define FLMR_PROF_RING 8

// ---- the batch plan: which kernel form runs at every stage (flmr_plan_batch below) --------------------------------------------
enum class s2_form : uint8_t { gather_f32, gather, xcd, walk, xcda };   // xcda: hi-only pass on the sliced kernel, band rescored by the gather
struct flmr_plan {
    bool sparse;            // compact score rows of the surviving centroids (fp16-split stage 0, one column tile) instead of the whole table
    flmr_s0_choice s0;      // stage-0 kernel and its partial-list geometry
    bool hi_first;          // stage 0 writes the "hi first" bounds q_err / q_err_sum
    bool chunked;           // candidates by the chunked kernel (else FLMR_CAND_IMPL=atomic)
    bool hits;              // hit prefilter
    bool scatter;           // stage 1 by list scatter for the queries it takes (hit_valid)
    bool fast;              // cand_plan_kernel plans the fast forms (and decides the dense modes); else the slot form
    int32_t img_rows;       // score-row images of the dense image form (0: it does not run)
    bool dense, exact_too;  // the dense stage-1 forms run; the exact form also takes the queries beyond the images
    bool qualifying;        // qualifying_kernel runs: nqual, row_ovf and the compact rows are this batch's
    bool recompute;         // the recompute form for queries over the score-row capacity
    bool modes;             // s1_dense_modes_kernel runs (mode / scan_skip needed and not made by cand_plan_kernel)
    bool scan;              // the code-scanning stage 1 runs for the queries no other form took
    s2_form s2;
    s2_sw s2_gather;        // the row-gather kernel's form
    s3_form s3;
};

// ---- the workspace record: every device buffer of a searcher, with what FLMR_POISON does to it ---------------------------------
// scratch: no batch may read what an earlier batch left in it.  FLMR_POISON fills the WHOLE allocation at the start of every batch
//          and of every phase 1 -- WS_FF: floats, halves and 64-bit keys get 0xFF bytes (NaNs; keys above every real key that carry
//          pid -1); WS_ZERO: counts, offsets, ranks, ids, flags and bit masks get 0, in range for every consumer (a query that lives
//          off them loses its survivors, which the result shows).
// carried: state that legitimately outlives a batch; never poisoned (the reason stands at the allocation).
enum ws_kind : uint8_t { WS_FF, WS_ZERO, WS_CARRIED };
struct ws_rec {
    void* ptr;
    size_t bytes;
    ws_kind kind;
    size_t phase_row;   // > 0: no phase reads what an earlier phase left in it either -- phases 2 / 3 fill the batch's rows of this many bytes
};
#define FLMR_WS_MAX 64

struct flmr_searcher {
    const flmr_index* ix;
    ws_rec ws[FLMR_WS_MAX]; int32_t nws;   // every device buffer below: what destroy frees and what the poison walks
    int32_t max_queries, max_nq;
    flmr_search_params_t maxp;
    int32_t ncol_max, idx_words, nblk, max_cells, nc_bucket;
    int64_t bitmap_words, cand_cap, bytes;
    float* cs; uint32_t* idx_bits; float* part_val; int32_t* part_idx; int32_t* cells; int32_t* ncell;
    uint32_t* bitmap; int32_t* cand; int32_t* cand_count; uint64_t* keys1; int32_t* s1_pids; int32_t* s1_count;
    uint64_t* keys2; int32_t* s2_pids; int32_t* s2_count; uint64_t* keys3; float* doc_scores;
    int32_t* overflow;          // = status: device flags [0] candidate capacity exceeded, [1] q_lens outside [0, nq] ([2], [3] unused)
    int32_t* row_ovf;           // [max_queries] 1 = more surviving centroids than compact score rows (row_cap): the query's stage 1 is
                                // recomputed from the fp16 centroids inside the same batch (no error, no host round trip)
    int32_t* status_host;       // pinned copy of the flags, refreshed asynchronously after every batch
    float* rows;                // compact score rows [max_queries, row_cap, 32]: the sparse path's whole "score table"
    uint32_t* idx_prefix;       // [max_queries, idx_words] ranks of the surviving centroids (qualifying_kernel)
    int32_t row_cap;            // score rows per query: min(K, FLMR_ROW_CAP (default 16384))
    hipEvent_t status_ev; bool status_pending;
    int32_t* q_lens_ws;         // [max_queries] query lengths clamped to [0, nq]: what every kernel reads
    flmr_options opt;           // variant switches, snapshot taken at flmr_searcher_create
    _Float16* q_hi; _Float16* q_lo;
    float* q_err;               // [max_queries, ncol_max] per-column error bound of the hi-only stage-0 scores
    float* q_err_sum;           // [max_queries] error bound of a passage's hi-only stage-2 score
    int32_t* s2_band; int32_t* s2_band_count; int32_t* s2_need; int32_t* s2_def; uint64_t* keys2b;   // stage 2, approximate-then-refine
    uint32_t* hit_bits; int32_t* hit_valid; int32_t* key_count; int32_t* chunk_hits;
    int32_t* s1_slot; int32_t* s2_slot;   // sharded protocol: position of each local survivor / finalist in the global list
    float* s2_part;             // XCD-sliced stage 2: per (query, slice, survivor) column maxima (NULL when the index has no split table)
    _Float16* q3_hi; _Float16* q3_lo;
    uint2* s3_desc; int64_t s3_desc_stride; int32_t* s3_wbeg; int32_t s3_wcap;   // planned-tile S3 (NULL: the passage-walking kernel)
    float* s3_colmax; int64_t s3_colmax_cap;   // long queries: per (query, finalist, column) maxima of the query-stationary S3 kernel
    int32_t* qual; int32_t* nqual; int32_t* chunk_cnt; uint8_t* cand_hit; int32_t qmax;
    // stage 1 for dense survivor sets (flmr_stage1_dense.hip): per query which form, the band of an image query, its error bound,
    // how many keys the selection reads, and which queries are left to the round-5 scan
    int32_t* s1d_any; int32_t* s1d_mode; int32_t* s1d_band; int32_t* s1d_band_count; float* s1d_err; int32_t* s1d_in_count; int32_t* s1d_scan_skip;
    int32_t s1d_img_rows;       // score-row images the LDS form holds (0: no dense form on this index)
    int32_t* cand_implied;      // flmr_cand_args::implied ([max_queries])
    int32_t* cand_fast;         // flmr_cand_args::fast_state ([FLMR_FAST_HDR + 2 * max_queries]; the header words live as long as the searcher)
    // last call (for taps)
    int32_t last_nqueries, last_ncol, last_ndocs;
    flmr_plan last_plan;        // what the last call ran
    flmr_cand_args last_ca{};   // candidate-stage arguments of the last batch (lazy FLMR_TAP_CANDIDATES in scatter mode)
    bool last_cand_lazy;        // the last batch's list-scatter forms skipped the ascending candidate lists (built on FLMR_TAP_CANDIDATES)
    hipStream_t last_stream;
    bool profiling;
    bool full_table;  // keep the whole centroid-score table (needed by the CENTROID_SCORES tap / retrieve())
    int32_t numerics; // FLMR_NUMERICS_CPU (default) | FLMR_NUMERICS_GPU_FP16
    // stage timing: a ring of event sets, one per profiled call, folded into acc_ms when read (or when the ring wraps)
    hipEvent_t ev[FLMR_PROF_RING][FLMR_NUM_STAGES + 1];
    int ev_first = 0, ev_pending = 0;   // oldest unread set, number of unread sets
    float acc_ms[FLMR_NUM_STAGES] = {};
    bool have_ms;
};

static int nc_bucket_of(int ncells) { return ncells <= 1 ? 1 : ncells <= 2 ? 2 : ncells <= 4 ? 4 : 8; }

// One workspace buffer: allocated, counted and recorded with its kind.  `phase_rows`: see ws_rec::phase_row (count / phase_rows
// elements per query).  A failed hipMalloc leaves *p NULL and no record: the optional buffers' callers go on without them.
template <typename T>
static int ws_alloc(flmr_searcher* s, T** p, size_t count, ws_kind kind, size_t phase_rows = 0) {
    const size_t bytes = (count ? count : 1) * sizeof(T);
    *p = nullptr;
    if (s->nws >= FLMR_WS_MAX) FLMR_FAIL(FLMR_ERR_INVALID, "workspace record full (FLMR_WS_MAX=%d)", FLMR_WS_MAX);
    FLMR_HIP(hipMalloc(reinterpret_cast<void**>(p), bytes));
    s->bytes += (int64_t)bytes;
    s->ws[s->nws++] = ws_rec{*p, bytes, kind, phase_rows ? bytes / phase_rows : 0};
    return FLMR_OK;
}
template <typename T>
static bool ws_alloc_optional(flmr_searcher* s, T** p, size_t count, ws_kind kind) {
    if (ws_alloc(s, p, count, kind) == FLMR_OK) return true;
    (void)hipGetLastError();
    *p = nullptr;
    return false;
}
static void ws_release_last(flmr_searcher* s) {   // (an optional buffer whose companion could not be had)
    const ws_rec& r = s->ws[--s->nws];
    (void)hipFree(r.ptr);
    s->bytes -= (int64_t)r.bytes;
}

// FLMR_POISON: the walk over the record.  `first_phase`: the call starts a batch (flmr_search_batch, phase 1, the probe) -- every
// scratch buffer, whole; else (phase 2 / 3) only the buffers no phase hands on, the batch's rows
static int ws_poison(flmr_searcher* s, int32_t nqueries, bool first_phase, hipStream_t st) {
    for (int i = 0; i < s->nws; i++) {
        const ws_rec& r = s->ws[i];
        if (r.kind == WS_CARRIED || !(first_phase || r.phase_row)) continue;
        FLMR_HIP(hipMemsetAsync(r.ptr, r.kind == WS_FF ? 0xFF : 0, first_phase ? r.bytes : (size_t)nqueries * r.phase_row, st));
    }
    return FLMR_OK;
}

static int check_params(const flmr_search_params_t* p) {
    if (!p) FLMR_FAIL(FLMR_ERR_INVALID, "params is NULL");
    if (p->ncells < 1 || p->ncells > FLMR_MAX_NCELLS) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "ncells=%d (1..%d)", p->ncells, FLMR_MAX_NCELLS);
    if (p->ndocs < 4 || p->ndocs > FLMR_MAX_NDOCS) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "ndocs=%d (4..%d)", p->ndocs, FLMR_MAX_NDOCS);
    if (p->nq_cand < 1 || p->nq_cand > FLMR_MAX_NQ_CAND) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "nq_cand=%d (1..%d)", p->nq_cand, FLMR_MAX_NQ_CAND);
    if (p->k < 1) FLMR_FAIL(FLMR_ERR_INVALID, "k=%d", p->k);
    return FLMR_OK;
}

extern "C" int flmr_searcher_create(const flmr_index_t* ix, int32_t max_queries, int32_t max_nq,
                                    const flmr_search_params_t* maxp, flmr_searcher_t** out) {
    if (!ix || !out) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    *out = nullptr;
    int rc = check_params(maxp);
    if (rc) return rc;
    if (max_queries < 1 || max_nq < 1) FLMR_FAIL(FLMR_ERR_INVALID, "max_queries/max_nq must be >= 1");
    flmr_options opt;
    rc = flmr_process_options(&opt);
    if (rc) return rc;
    flmr_searcher* s = new (std::nothrow) flmr_searcher();
    if (!s) FLMR_FAIL(FLMR_ERR_NOMEM, "host allocation failed");
    memset(s, 0, sizeof(*s));
    s->ix = ix; s->max_queries = max_queries; s->max_nq = max_nq; s->maxp = *maxp;
    s->opt = opt;
    const int nqc = maxp->nq_cand < max_nq ? maxp->nq_cand : max_nq;
    s->ncol_max = (int32_t)flmr_round_up(nqc, 32);
    s->idx_words = (int32_t)flmr_ceil_div(ix->K, 32);
    s->nblk = (int32_t)flmr_ceil_div(ix->K, 64);  // upper bound on partial-list blocks (64 rows each on the fp16 kernels, 128 on the fp32 ones)
    s->max_cells = nqc * maxp->ncells;
    s->nc_bucket = nc_bucket_of(maxp->ncells);
    s->bitmap_words = flmr_ceil_div(ix->num_passages > 0 ? ix->num_passages : 1, 32);
    const int mc = s->max_cells < ix->K ? s->max_cells : ix->K;
    s->cand_cap = ix->ivf_len_prefix[mc] < ix->num_passages ? ix->ivf_len_prefix[mc] : ix->num_passages;
    if (s->cand_cap < 1) s->cand_cap = 1;
    const size_t B = (size_t)max_queries;
    const int nd = maxp->ndocs, nd4 = maxp->ndocs / 4;
    // WS(buffer, elements, kind[, B]): the kind is the buffer's FLMR_POISON class (ws_kind above); a trailing B marks the six buffers
    // FLMR_POISON has filled since round 4, which phases 2 / 3 fill too (their pattern stays 0xFF, ranks and ids included: no
    // consumer reads them before their writer in any phase)
#define WS(ptr, count, ...)                                  \
    do {                                                     \
        rc = ws_alloc(s, &s->ptr, (count), __VA_ARGS__);     \
        if (rc) { flmr_searcher_destroy(s); return rc; }     \
    } while (0)
    // The full K x ncol score table per query (16.8 MB at K = 131072) is allocated on first use by a batch that needs it
    // (full-table mode: taps / retrieve(), centroids that are not fp16-exact, nq_cand > 32); the default path keeps only the
    // rows of each query's surviving centroids, at most row_cap of them (2 MB per query at the default).
    s->cs = nullptr;
    {
        const int32_t cap = s->opt.row_cap ? s->opt.row_cap : 16384;   // (at most 65535: the code-scanning stage 1 keeps 16-bit ranks in LDS)
        s->row_cap = cap < ix->K ? cap : ix->K;
    }
    // stage 0 -> candidates -> stage 1.  Everything a phase hands on (q_hi / q_lo to phase 2, the status words) or a tap reads
    // after the batch (idx_bits, cells, cand, the survivor lists, doc_scores, the form words) stays valid until the next batch or
    // phase 1 starts: that is where the scratch kinds are filled, so none of them needs the carried kind.
    WS(rows, B * (size_t)s->row_cap * 32, WS_FF, B);            // float score rows
    WS(idx_prefix, B * (size_t)s->idx_words, WS_FF, B);         // ranks (the round-4 pattern)
    WS(idx_bits, B * (size_t)s->idx_words, WS_ZERO);            // centroid mask: no survivor
    WS(part_val, B * (size_t)s->nblk * s->ncol_max * s->nc_bucket, WS_FF);     // float block maxima / list values
    WS(part_idx, B * (size_t)s->nblk * s->ncol_max * s->nc_bucket, WS_ZERO);   // centroid ids (or the coarse maxima: 0.0f)
    WS(cells, B * (size_t)s->max_cells, WS_ZERO);               // centroid ids
    WS(ncell, B, WS_ZERO);
    WS(bitmap, B * (size_t)s->bitmap_words, WS_ZERO);           // passage mask
    WS(cand, B * (size_t)s->cand_cap, WS_ZERO);                 // pids
    WS(cand_count, B, WS_ZERO);
    WS(keys1, B * (size_t)s->cand_cap, WS_FF, B);
    WS(s1_pids, B * (size_t)nd, WS_ZERO);
    WS(s1_count, B, WS_ZERO);
    WS(keys2, B * (size_t)nd, WS_FF, B);
    WS(s2_pids, B * (size_t)nd4, WS_ZERO);
    WS(s2_count, B, WS_ZERO);
    WS(keys3, B * (size_t)nd4, WS_FF, B);
    WS(doc_scores, B * (size_t)nd4, WS_FF);                     // float
    WS(overflow, 4, WS_CARRIED);                                // the deferred status: raised by a batch, read and cleared by a later call
    WS(q_lens_ws, B, WS_ZERO);                                  // lengths in [0, nq] (filled BEFORE the batch's lengths are written)
    WS(q_hi, B * (size_t)s->ncol_max * FLMR_DIM, WS_FF);        // halves; phase 1's images are phase 2's
    WS(q_lo, B * (size_t)s->ncol_max * FLMR_DIM, WS_FF);
    WS(q_err, B * (size_t)s->ncol_max, WS_FF);                  // float bounds
    WS(q_err_sum, B, WS_FF);
    WS(s2_band, B * (size_t)nd, WS_ZERO);                       // pids
    WS(s2_band_count, B, WS_ZERO);
    WS(s2_need, B, WS_ZERO);
    WS(s2_def, B, WS_ZERO);
    WS(keys2b, B * (size_t)nd, WS_FF);
    WS(hit_bits, B * (size_t)s->bitmap_words, WS_ZERO);         // passage mask
    WS(hit_valid, B, WS_ZERO);                                  // flag: 0 = not a list-scatter query
    WS(key_count, B, WS_ZERO);
    WS(s1_slot, B * (size_t)nd, WS_ZERO);                       // positions in the global lists (written and read inside one phase)
    WS(s2_slot, B * (size_t)nd4, WS_ZERO);
    if (ix->doc_splits && s->ncol_max == 32 && (flmr_stage2_xcd_pays(ix) || s->opt.s2 == s2_sw::xcd)) {
        // optional: without it (1 KB per query and survivor; e.g. out of memory) stage 2 runs in its gather form
        (void)ws_alloc_optional(s, &s->s2_part, flmr_stage2_xcd_part_floats(ix, (int64_t)B, nd), WS_FF);   // float column maxima
    }
    s->qmax = s->row_cap;
    WS(qual, B * (size_t)s->qmax, WS_FF, B);                    // centroid ids (the round-4 pattern)
    WS(nqual, B, WS_ZERO);
    WS(chunk_cnt, B * (size_t)ix->nchunks, WS_ZERO);
    WS(chunk_hits, B * (size_t)ix->nchunks, WS_ZERO);
    WS(cand_hit, B * (size_t)s->cand_cap, WS_ZERO);             // byte flags
    // dense stage 1: needs the sorted code copy (whole 16-byte pieces are read: its padding) and 32-bit token offsets
    s->s1d_img_rows = (ix->codes_sorted && s->ncol_max == 32 && s->opt.s1 != s1_sw::scan) ? flmr_s1_dense_image_rows(max_queries, s->idx_words, ix->mean_ulen) : 0;
    WS(s1d_any, 16, WS_ZERO);                                   // flags + item counters: no query takes a dense pass
    WS(s1d_mode, B, WS_ZERO);                                   // FLMR_S1D_SKIP
    WS(s1d_band_count, B, WS_ZERO);
    WS(s1d_err, B, WS_FF);                                      // float
    WS(s1d_in_count, B, WS_ZERO);
    WS(s1d_scan_skip, B, WS_ZERO);
    WS(row_ovf, B, WS_ZERO);                                    // flag
    if (s->s1d_img_rows > 0) WS(s1d_band, B * (size_t)s->cand_cap, WS_ZERO);   // pids
    WS(q3_hi, B * (size_t)flmr_round_up(max_nq, 32) * FLMR_DIM, WS_FF);        // halves
    WS(q3_lo, B * (size_t)flmr_round_up(max_nq, 32) * FLMR_DIM, WS_FF);
    {   // optional workspace of the planned-tile S3 kernel: one 8-byte descriptor per 32-token tile of a query's finalists
        s->s3_desc_stride = (int64_t)nd4 * ((ix->max_doclen + 31) / 32);
        s->s3_wcap = nd4 + 8;
        const size_t db = B * (size_t)s->s3_desc_stride * sizeof(uint2);
        if (s->s3_desc_stride > 0 && db <= ((size_t)1 << 30) && ws_alloc_optional(s, &s->s3_desc, B * (size_t)s->s3_desc_stride, WS_ZERO) &&   // (token offset, slot)
            !ws_alloc_optional(s, &s->s3_wbeg, B * (size_t)s->s3_wcap, WS_ZERO)) {                                                            // tile offsets
            ws_release_last(s);   // both or neither
            s->s3_desc = nullptr;
        }
        if (s->s3_desc && max_nq > 32) {
            s->s3_colmax_cap = (int64_t)B * nd4 * flmr_round_up(max_nq, 32) + (int64_t)B;   // (+ the per-query output scales of the query-stationary kernel)
            if (s->s3_colmax_cap * (int64_t)sizeof(float) > ((int64_t)2 << 30) ||
                !ws_alloc_optional(s, &s->s3_colmax, (size_t)s->s3_colmax_cap, WS_FF))       // float column maxima
                s->s3_colmax_cap = 0;
        }
    }
    WS(cand_implied, B, WS_ZERO);                               // flag: 0 = the candidate bitmap is marked in the scatter pass
    // (plan words and key counters, written for every query of a batch before they are read; zeroed once here as before)
    WS(cand_fast, 2 * B + FLMR_FAST_HDR, WS_ZERO);
#undef WS
    FLMR_HIP(hipMemset(s->cand_fast, 0, (2 * B + FLMR_FAST_HDR) * sizeof(int32_t)));
    FLMR_HIP(hipMemset(s->overflow, 0, 4 * sizeof(int32_t)));
    FLMR_HIP(hipHostMalloc(reinterpret_cast<void**>(&s->status_host), 4 * sizeof(int32_t), hipHostMallocDefault));
    s->status_host[0] = s->status_host[1] = s->status_host[2] = s->status_host[3] = 0;
    FLMR_HIP(hipEventCreateWithFlags(&s->status_ev, hipEventDisableTiming));
    for (int r = 0; r < FLMR_PROF_RING; r++)
        for (int i = 0; i <= FLMR_NUM_STAGES; i++) FLMR_HIP(hipEventCreate(&s->ev[r][i]));
    *out = s;
    return FLMR_OK;
}

extern "C" int flmr_searcher_destroy(flmr_searcher_t* s) {
    if (!s) return FLMR_OK;
    for (int i = 0; i < s->nws; i++) (void)hipFree(s->ws[i].ptr);
    if (s->status_host) (void)hipHostFree(s->status_host);
    if (s->status_ev) (void)hipEventDestroy(s->status_ev);
    for (int r = 0; r < FLMR_PROF_RING; r++)
        for (int i = 0; i <= FLMR_NUM_STAGES; i++)
            if (s->ev[r][i]) (void)hipEventDestroy(s->ev[r][i]);
    delete s;
    return FLMR_OK;
}

extern "C" int flmr_searcher_workspace_bytes(const flmr_searcher_t* s, int64_t* bytes) {
    if (!s || !bytes) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    *bytes = s->bytes;
    return FLMR_OK;
}

// waits for the oldest unread event set and adds its stage times to acc_ms
static int fold_oldest(flmr_searcher* s) {
    hipEvent_t* e = s->ev[s->ev_first];
    FLMR_HIP(hipEventSynchronize(e[FLMR_NUM_STAGES]));
    for (int i = 0; i < FLMR_NUM_STAGES; i++) {
        float ms = 0.f;
        FLMR_HIP(hipEventElapsedTime(&ms, e[i], e[i + 1]));
        s->acc_ms[i] += ms;
    }
    s->ev_first = (s->ev_first + 1) % FLMR_PROF_RING;
    s->ev_pending--;
    return FLMR_OK;
}

extern "C" int flmr_searcher_set_profiling(flmr_searcher_t* s, int32_t enable) {
    if (!s) FLMR_FAIL(FLMR_ERR_INVALID, "NULL searcher");
    if (s->profiling != (enable != 0)) {   // a change of mode starts a fresh accumulation
        s->ev_pending = 0;
        s->have_ms = false;
        for (float& v : s->acc_ms) v = 0.f;
    }
    s->profiling = enable != 0;
    return FLMR_OK;
}

extern "C" int flmr_searcher_set_full_table(flmr_searcher_t* s, int32_t enable) {
    if (!s) FLMR_FAIL(FLMR_ERR_INVALID, "NULL searcher");
    s->full_table = enable != 0;
    return FLMR_OK;
}

// The smallest fp32 x with half(x) >= half(thr): the reference's CUDA path compares an fp16 tensor with the Python scalar
// (index_storage.py:116 on `centroid_scores.cuda()` half values: the scalar is taken in the tensor's dtype), so the
// predicate on the fp32-accumulated score s is  half(s) >= half(thr)  <=>  s >= that x (rounding is monotone).
static float f16_threshold(float thr) {
    const _Float16 h = (_Float16)thr;
    if (!(h == h)) return thr;
    uint16_t hb;
    memcpy(&hb, &h, 2);
    if ((hb & 0x7fffu) == 0) {   // +-0: anything that rounds to (+-)0 or above
        hb = 0x8001u;            // largest negative subnormal half = predecessor of zero
    } else if (hb & 0x8000u) {
        hb++;                    // negative: predecessor = larger magnitude
    } else {
        hb--;                    // positive: predecessor = smaller magnitude
    }
    _Float16 pred;
    memcpy(&pred, &hb, 2);
    const float mid = 0.5f * ((float)pred + (float)h);   // exact in fp32 (two adjacent halves)
    // the midpoint rounds to the neighbour with the even mantissa
    uint16_t hbits;
    memcpy(&hbits, &h, 2);
    const bool h_even = (hbits & 1u) == 0;
    return h_even ? mid : nextafterf(mid, INFINITY);
}

extern "C" int flmr_searcher_set_numerics(flmr_searcher_t* s, int32_t mode) {
    if (!s) FLMR_FAIL(FLMR_ERR_INVALID, "NULL searcher");
    if (mode != FLMR_NUMERICS_CPU && mode != FLMR_NUMERICS_GPU_FP16) FLMR_FAIL(FLMR_ERR_INVALID, "unknown numerics mode %d", mode);
    if (mode == FLMR_NUMERICS_GPU_FP16 && !(s->ix->centroids_f16_exact && s->ix->centroids_f16 && s->ix->K % 64 == 0))
        FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "the fp16 numerics mode needs fp16-representable centroids (every reference-format index) and K %% 64 == 0");
    s->numerics = mode;
    return FLMR_OK;
}

extern "C" int flmr_searcher_stage_ms(flmr_searcher_t* s, float* ms) {
    if (!s || !ms) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    if (!s->have_ms) FLMR_FAIL(FLMR_ERR_INVALID, "no profiled flmr_search_batch call since the last read");
    while (s->ev_pending) {
        const int rc = fold_oldest(s);
        if (rc) return rc;
    }
    for (int i = 0; i < FLMR_NUM_STAGES; i++) {
        ms[i] = s->acc_ms[i];
        s->acc_ms[i] = 0.f;
    }
    s->have_ms = false;
    return FLMR_OK;
}

// ---- one batch = a context (validated parameters + kernel argument blocks) run through stage helpers -----------------
struct run_ctx {
    flmr_searcher* s;
    const float* Q;
    const int32_t* q_lens;
    int32_t nqueries, nq, nqc, ncol;
    flmr_search_params_t p;
    bool sparse;
    hipStream_t st;
    flmr_s0_args a0{};
    flmr_filter_args f{};
    flmr_plan plan;
    int stage;  // profiling event cursor
    int ev_set; // event set of this call
};

#define RUN(x)          \
    do {                \
        int rc__ = (x); \
        if (rc__) return rc__; \
    } while (0)

static int mark(run_ctx& c) {
    if (c.s->profiling && c.stage <= FLMR_NUM_STAGES) FLMR_HIP(hipEventRecord(c.s->ev[c.ev_set][c.stage], c.st));
    c.stage++;
    return FLMR_OK;
}

// Device-side error flags (candidate capacity, q_lens range) are copied to pinned host memory after every batch without a
// sync; the next call on the searcher (or flmr_searcher_check, which waits) reports a raised flag and clears it.
static int poll_status(flmr_searcher* s, bool wait) {
    if (!s->status_pending) return FLMR_OK;
    if (wait) {
        FLMR_HIP(hipEventSynchronize(s->status_ev));
    } else {
        const hipError_t e = hipEventQuery(s->status_ev);
        if (e == hipErrorNotReady) return FLMR_OK;
        FLMR_HIP(e);
    }
    s->status_pending = false;
    const int32_t ovf = s->status_host[0], bad = s->status_host[1];
    if (ovf || bad) {
        s->status_host[0] = s->status_host[1] = s->status_host[2] = 0;
        // cleared IN ORDER on the searcher's stream: a synchronous memset on the null stream is not ordered against a later
        // batch already running on a non-blocking stream and could wipe that batch's flag
        FLMR_HIP(hipMemsetAsync(s->overflow, 0, 4 * sizeof(int32_t), s->last_stream));
        if (ovf)
            FLMR_FAIL(FLMR_ERR_CAPACITY, "an earlier batch produced more candidates than the workspace bound (cand_cap=%lld): its "
                      "candidate lists were truncated and its results are not reliable (is the IVF consistent with the codes?)",
                      (long long)s->cand_cap);
        FLMR_FAIL(FLMR_ERR_INVALID, "an earlier batch passed q_lens outside [0, nq]; they were clamped");
    }
    return FLMR_OK;
}

static int push_status(run_ctx& c) {
    flmr_searcher* s = c.s;
    FLMR_HIP(hipMemcpyAsync(s->status_host, s->overflow, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c.st));
    FLMR_HIP(hipEventRecord(s->status_ev, c.st));
    s->status_pending = true;
    return FLMR_OK;
}

extern "C" int flmr_searcher_status_async(flmr_searcher_t* s, int32_t* host_flags, flmr_stream_t stream) {
    if (!s || !host_flags) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    FLMR_HIP(hipMemcpyAsync(host_flags, s->overflow, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, reinterpret_cast<hipStream_t>(stream)));
    return FLMR_OK;
}

extern "C" int flmr_searcher_check(flmr_searcher_t* s) {
    if (!s) FLMR_FAIL(FLMR_ERR_INVALID, "NULL searcher");
    return poll_status(s, true);
}

__global__ void sanitize_q_lens_kernel(const int32_t* in, int32_t n, int32_t nq, int32_t* out, int32_t* flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t v = in[i];
    const int32_t c = v < 0 ? 0 : (v > nq ? nq : v);
    out[i] = c;
    if (c != v) atomicExch(flag, 1);
}

// the sparse score table + recomputing stage 2 (and with them the query-split stage 0) need the fp16-split S0 path and
// a single column tile
static bool sparse_path(const flmr_searcher* s, int ncol) {
    const flmr_index* ix = s->ix;
    const flmr_options& o = s->opt;
    const bool f16_path = ix->centroids_f16_exact && ix->centroids_f16 && (ix->K % 64 == 0) && o.s0 != s0_sw::f32 && o.s0 != s0_sw::valu;
    return f16_path && ncol == 32 && !s->full_table && !o.full_table;
}

extern "C" int flmr_searcher_probe_supported(const flmr_searcher_t* s, int32_t nq, const flmr_search_params_t* p,
                                             int32_t* supported) {
    if (!s || !p || !supported) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    const int nqc = p->nq_cand < nq ? p->nq_cand : nq;
    *supported = sparse_path(s, (int)flmr_round_up(nqc, 32)) ? 1 : 0;
    return FLMR_OK;
}

// the stage-3 arguments of a call (`s0_images`: stage 0 of THIS call split the same queries -- flmr_search_batch, not the phases)
static flmr_maxsim_args s3_args(const run_ctx& c, bool s0_images) {
    flmr_searcher* s = c.s;
    flmr_maxsim_args m{};
    m.ix = s->ix; m.Q = c.Q; m.q_lens = c.q_lens; m.nqueries = c.nqueries; m.nq = c.nq;
    m.pids = s->s2_pids; m.pid_stride = s->maxp.ndocs / 4; m.counts = s->s2_count; m.max_count = c.p.ndocs / 4;
    m.keys = s->keys3; m.key_stride = s->maxp.ndocs / 4; m.scores = s->doc_scores;
    m.q_hi = s->q3_hi; m.q_lo = s->q3_lo;
    m.gpu_fp16 = c.f.f16_round;
    m.plan_desc = s->s3_desc; m.plan_stride = s->s3_desc_stride; m.plan_wbeg = s->s3_wbeg; m.plan_wcap = s->s3_wcap;
    m.colmax_ws = s->s3_colmax; m.colmax_cap = s->s3_colmax_cap;
    // Stage 0's fp16 images ARE stage 3's when every query row is a candidate-generation column (nq <= 32 <= nq_cand): rows
    // below min(q_len, nq) real, the rest zero, one tile of 32 -- no second split launch
    if (s0_images && c.sparse && !c.f.f16_round && c.nq <= 32 && c.nqc == c.nq && c.ncol == 32) {
        m.q_hi = s->q_hi; m.q_lo = s->q_lo;
        m.q_split_done = 1;
    }
    return m;
}

// The plan of one call: every stage's kernel form, from the searcher's switch snapshot, the index, the workspace and the batch.
// `whole_batch`: flmr_search_batch.  Phase 2 of the sharded protocol scores only this shard's members (a fraction of ndocs per
// query): the table walk, whose cost does not shrink with the number of survivors, is then the wrong form unless forced; so is the
// XCD-sliced kernel, whose waves each take one eighth of 64 survivors' tokens (per-rank compute of a step at 8 shards,
// profiles/shard_step_model.py: 2.16 ms sliced, 1.92 ms gather).  Also applies the stage-0 geometry to c.a0.
static void plan_batch(run_ctx& c, bool whole_batch) {
    flmr_searcher* s = c.s;
    const flmr_index* ix = s->ix;
    const flmr_options& o = s->opt;
    flmr_plan& pl = c.plan;
    pl = flmr_plan{};
    pl.sparse = c.sparse;
    // stage 0 (the block maxima of the row-stationary kernels are the full values: s0_select_cells must not assume otherwise)
    pl.s0 = flmr_s0_choose(c.a0, o);
    c.a0.nblk = pl.s0.nblk; c.a0.part_rows = pl.s0.part_rows; c.a0.grp_blocks = pl.s0.grp_blocks;
    if (pl.s0.form == s0_form::f16_sparse || pl.s0.form == s0_form::f16_table) { c.a0.q_err = nullptr; c.a0.q_err_buf = nullptr; }
    pl.hi_first = (pl.s0.form == s0_form::qs || pl.s0.form == s0_form::qs2) && c.a0.q_err_buf != nullptr;
    // stage 1: the list scatter (single column tile, sparse or full table alike) for the queries it takes; the dense forms of
    // flmr_stage1_dense.hip (sparse path, one column tile, CPU-path numerics) for those it leaves; the recompute form for queries over
    // the score-row capacity; the code-scanning kernel for the rest (every query under FLMR_S1_IMPL=scan)
    pl.chunked = !o.cand_atomic;
    pl.hits = !o.s1_no_hitmap;
    pl.scatter = pl.chunked && pl.hits && c.ncol == 32 && o.s1 != s1_sw::scan;
    pl.fast = pl.scatter && o.s1 != s1_sw::slots;
    pl.dense = s->s1d_img_rows > 0 && pl.chunked && c.sparse && c.ncol == 32 && !c.f.f16_round && o.s1 != s1_sw::scan;
    pl.img_rows = pl.dense ? s->s1d_img_rows : 0;
    pl.exact_too = pl.dense && o.s1 != s1_sw::image;   // (development: "image" leaves the queries beyond the images to the scan)
    pl.qualifying = pl.chunked || c.sparse;
    pl.recompute = c.sparse && s->row_cap < ix->K;
    pl.scan = !(pl.dense && pl.exact_too);   // (with both dense forms on, every query the list scatter leaves is theirs or the recompute form's)
    pl.modes = !pl.fast && (pl.dense || pl.scatter || pl.recompute);   // (else the scan takes every query: no skip list)
    // stage 2
    const bool walk_pays = ix->codes_sorted && ix->centroids_f16_tiled && flmr_stage2_walk_pays(ix, c.nqueries, c.p.ndocs);
    const bool dflt = o.s2 == s2_sw::dflt;
    const bool walk = c.sparse && !c.f.f16_round && ix->codes_sorted && ix->centroids_f16_tiled &&
                      (o.s2 == s2_sw::walk || (dflt && whole_batch && walk_pays));
    const bool xcd = !walk && c.sparse && s->s2_part && c.f.ncol == 32 && (o.s2 == s2_sw::xcd || (dflt && whole_batch && flmr_stage2_xcd_pays(ix)));
    pl.s2 = xcd ? s2_form::xcd : walk ? s2_form::walk : c.sparse ? s2_form::gather : s2_form::gather_f32;
    // default on the sliced kernel (the batch's error bounds at hand): hi-only pass, plan, full rescoring of the band by the gather
    // kernel, finish (flmr_filter.hip) -- the same SET as the sorted form; any other FLMR_S2_IMPL keeps the full scores and the sorted list
    if (whole_batch && pl.hi_first && s->s2_part && (o.s2 == s2_sw::xcda || (dflt && flmr_stage2_xcd_pays(ix) && !walk_pays)))
        pl.s2 = s2_form::xcda;
    pl.s2_gather = (o.s2 == s2_sw::regs || o.s2 == s2_sw::ldsb) ? o.s2 : s2_sw::lds;
    // stage 3
    pl.s3 = flmr_s3_choose(s3_args(c, whole_batch), o);
}

static int prepare_ctx(run_ctx& c, flmr_searcher* s, const float* Q, const int32_t* q_lens, int32_t nqueries, int32_t nq,
                       const flmr_search_params_t* p, flmr_stream_t stream, bool whole_batch = false, bool first_phase = true) {
    if (!s || !Q) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    RUN(check_params(p));
    RUN(poll_status(s, false));
    if (nqueries < 1 || nqueries > s->max_queries) FLMR_FAIL(FLMR_ERR_CAPACITY, "nqueries=%d > max_queries=%d", nqueries, s->max_queries);
    if (nq < 1 || nq > s->max_nq) FLMR_FAIL(FLMR_ERR_CAPACITY, "nq=%d > max_nq=%d", nq, s->max_nq);
    const int nqc = p->nq_cand < nq ? p->nq_cand : nq;
    const int ncol = (int)flmr_round_up(nqc, 32);
    if (ncol > s->ncol_max || nqc * p->ncells > s->max_cells || nc_bucket_of(p->ncells) > s->nc_bucket || p->ndocs > s->maxp.ndocs)
        FLMR_FAIL(FLMR_ERR_CAPACITY, "params exceed the bounds given at flmr_searcher_create");
    const flmr_index* ix = s->ix;
    c.s = s; c.Q = Q; c.q_lens = q_lens; c.nqueries = nqueries; c.nq = nq; c.nqc = nqc; c.ncol = ncol; c.p = *p;
    c.st = reinterpret_cast<hipStream_t>(stream);
    c.stage = 0;
    if (s->profiling && s->ev_pending == FLMR_PROF_RING) RUN(fold_oldest(s));   // the ring is full: make room (waits)
    c.ev_set = (s->ev_first + s->ev_pending) % FLMR_PROF_RING;
    c.sparse = sparse_path(s, ncol);
    if (!c.sparse && !s->cs) {   // first batch that needs the whole K x ncol table per query: allocate it now (synchronous, once)
        const size_t bytes = (size_t)s->max_queries * (size_t)ix->K * s->ncol_max * sizeof(float);
        if (!ws_alloc_optional(s, &s->cs, bytes / sizeof(float), WS_FF))   // float scores (FLMR_TAP_CENTROID_SCORES reads the last batch's)
            FLMR_FAIL(FLMR_ERR_NOMEM, "the full centroid-score table needs %.1f GB for %d queries (full-table mode: taps, centroids that are "
                      "not fp16-representable, nq_cand > 32): create the searcher for fewer queries", bytes / 1e9, s->max_queries);
    }
    // test runs: nothing may be read from an earlier batch's workspace (before anything of this call is written into it)
    if (s->opt.poison) RUN(ws_poison(s, nqueries, first_phase, c.st));
    if (q_lens) {  // kernels only ever see lengths inside [0, nq]; a violation is reported by the next status poll
        hipLaunchKernelGGL(sanitize_q_lens_kernel, dim3((nqueries + 255) / 256), dim3(256), 0, c.st, q_lens, nqueries, nq,
                           s->q_lens_ws, s->overflow + 1);
        FLMR_LAUNCH_CHECK();
        c.q_lens = q_lens = s->q_lens_ws;
    }
    flmr_s0_args& a0 = c.a0;
    a0.centroids = ix->centroids; a0.Q = Q; a0.q_lens = q_lens;
    a0.K = ix->K; a0.nqueries = nqueries; a0.nq = nq; a0.nq_cand = nqc; a0.ncol = ncol; a0.ncells = p->ncells;
    const bool f16num = s->numerics == FLMR_NUMERICS_GPU_FP16;
    a0.thr = f16num ? f16_threshold(p->centroid_score_threshold) : p->centroid_score_threshold;
    a0.q_hi_only = f16num ? 1 : 0;
    a0.cs = c.sparse ? nullptr : s->cs; a0.idx_bits = s->idx_bits; a0.idx_words = s->idx_words;
    a0.part_val = s->part_val; a0.part_idx = s->part_idx;
    a0.cells = s->cells; a0.ncell = s->ncell; a0.max_cells = s->max_cells;
    a0.q_hi = s->q_hi; a0.q_lo = s->q_lo; a0.centroids_f16_exact = ix->centroids_f16_exact;
    // "hi first" stage 0: on unless the fp16 numerics mode makes it moot (q_lo = 0) or FLMR_S0_IMPL asks for another kernel
    a0.q_err_buf = f16num ? nullptr : s->q_err;
    // (any batch size since the cell selection reads the coarse level of maxima this path leaves: a single-query call takes 0.309 ms
    // with it, 0.322 ms with both products everywhere; before the coarse level the selection's serial pass over a near-tie column
    // -- most queries have one -- made the shortcut a loss under 16 queries)
#ifndef S0_HIFIRST_MIN_QUERIES
#define S0_HIFIRST_MIN_QUERIES 1
#endif
    a0.q_err = (!f16num && (s->opt.s0 == s0_sw::dflt || s->opt.s0 == s0_sw::qs1) && nqueries >= S0_HIFIRST_MIN_QUERIES) ? s->q_err : nullptr;
    a0.q_err_sum = s->q_err_sum;
    a0.cen_norm_max = ix->cen_norm_max;
    a0.centroids_f16 = ix->centroids_f16;
    a0.full_table = c.sparse ? 0 : 1;
    flmr_filter_args& f = c.f;
    f.cs = c.sparse ? s->rows : s->cs; f.cs_query_stride = c.sparse ? (int64_t)s->row_cap * 32 : (int64_t)ix->K * ncol;
    f.cs_compact = c.sparse ? 1 : 0; f.row_cap = s->row_cap; f.idx_prefix = s->idx_prefix;
    f.K = ix->K; f.ncol = ncol; f.nq_cand = nqc;
    f.nqueries = nqueries; f.q_lens = q_lens; f.codes = ix->codes; f.doclens = nullptr; f.offsets = ix->doc_offsets;
    f.f16_round = f16num ? 1 : 0;
    f.ulen_sorted = ix->doc_ulen;
    plan_batch(c, whole_batch);
    s->last_nqueries = nqueries; s->last_ncol = ncol; s->last_ndocs = p->ndocs; s->last_stream = c.st;
    s->last_plan = c.plan;
    return FLMR_OK;
}

// S0 (scores, cells), candidates (+ hit flags), S1, top-ndocs selection -> s->s1_pids / s1_count (+ optional global keys)
static int stage_cand_s1(run_ctx& c, uint64_t* out_keys);

static int stage_s0_s1(run_ctx& c, uint64_t* out_keys) {
    hipStream_t st = c.st;
    RUN(mark(c));
    RUN(flmr_launch_centroid_scores(c.a0, c.plan.s0.form, st));
    RUN(mark(c));
    RUN(flmr_launch_select_cells(c.a0, st));
    RUN(mark(c));
    return stage_cand_s1(c, out_keys);
}

// candidates (+ hit flags), S1, top-ndocs selection, given idx_bits / cells / ncell (and the table rows of idx) in place
static int stage_cand_s1(run_ctx& c, uint64_t* out_keys) {
    flmr_searcher* s = c.s;
    const flmr_index* ix = s->ix;
    const flmr_plan& pl = c.plan;
    hipStream_t st = c.st;
    const int32_t* sel_counts = s->cand_count;
    flmr_cand_args ca{};
    {
        ca.nqueries = c.nqueries; ca.idx_words = s->idx_words; ca.max_cells = s->max_cells; ca.qmax = s->qmax;
        ca.nchunks = ix->nchunks; ca.words = s->bitmap_words; ca.cand_cap = s->cand_cap;
        ca.idx_bits = s->idx_bits; ca.cells = s->cells; ca.ncell = s->ncell;
        ca.ivf_pids = ix->ivf_pids; ca.ivf_offsets = ix->ivf_offsets; ca.chunk_tab = ix->ivf_chunk_tab;
        ca.qual = s->qual; ca.nqual = s->nqual; ca.hit_valid = s->hit_valid;
        ca.cand_bits = s->bitmap; ca.hit_bits = s->hit_bits; ca.chunk_cnt = s->chunk_cnt;
        ca.cand = s->cand; ca.cand_hit = s->cand_hit; ca.cand_count = s->cand_count; ca.overflow = s->overflow;
        ca.scatter = pl.scatter ? 1 : 0;
        ca.cs = c.f.cs; ca.cs_query_stride = c.f.cs_query_stride; ca.nq_cand = c.nqc; ca.q_lens = c.q_lens;
        ca.cs_compact = c.f.cs_compact; ca.idx_prefix = s->idx_prefix;
        ca.rows_out = c.sparse ? s->rows : nullptr; ca.cen16 = ix->centroids_f16; ca.q_hi = s->q_hi; ca.q_lo = s->q_lo;
        ca.keys = s->keys1; ca.key_count = s->key_count; ca.chunk_hits = s->chunk_hits; ca.n_select = c.p.ndocs;
        ca.f16_round = c.f.f16_round;
        ca.fast_state = s->opt.s1 == s1_sw::slots ? nullptr : s->cand_fast;
        ca.row_ovf = s->row_ovf;
        // who takes which query afterwards: the list-scatter forms (hit_valid), the dense forms, the recompute form (row_ovf), the scan
        // (the rest); decided per query by cand_plan_kernel when it runs, else by flmr_launch_s1_dense_modes below
        if (pl.fast) {
            ca.s1d_mode = s->s1d_mode; ca.s1d_scan_skip = s->s1d_scan_skip; ca.s1d_any = s->s1d_any;
            ca.s1d_img_rows = pl.img_rows;
            ca.s1d_exact_too = pl.exact_too ? 1 : 0;
            ca.implied = s->cand_implied; ca.force_bitmaps = s->opt.cand_bitmaps ? 1 : 0;
        }
    }
    if (pl.chunked) {
        RUN(flmr_launch_candidates_chunked(ca, st));
        s->last_ca = ca; s->last_cand_lazy = pl.scatter;
        RUN(mark(c));
        RUN(mark(c));  // (the hit set is produced by the same pass: the s1_hitmap stage is empty in this mode)
    } else {
        if (pl.qualifying) RUN(flmr_launch_qualifying(ca, st));   // (the compact score rows stage 1 reads)
        RUN(flmr_launch_ivf_mark(s->cells, s->ncell, s->max_cells, c.nqueries, ix->ivf_pids, ix->ivf_offsets, s->bitmap,
                                 s->bitmap_words, st));
        RUN(flmr_launch_compact(s->bitmap, s->bitmap_words, ix->num_passages, c.nqueries, s->cand, s->cand_cap,
                                s->cand_count, s->overflow, st));
        s->last_cand_lazy = false;
        RUN(mark(c));
        if (pl.hits)
            RUN(flmr_launch_hit_bitmap(s->idx_bits, s->idx_words, c.nqueries, ix->ivf_pids, ix->ivf_offsets, s->cand_count,
                                       s->hit_bits, s->bitmap_words, s->hit_valid, st));
        RUN(mark(c));
    }
    // Queries the list-scatter forms did not take (hit_valid == 0: more surviving centroids or longer lists than they handle):
    // the dense forms of flmr_stage1_dense.hip -- fp16 images of the query's score rows in LDS, upper-bound keys for every
    // candidate, the band around the cut rescored exactly -- where the rows fit (<= ~2 k survivors), the same kernel's exact form
    // beyond; the round-5 scan keeps the cases those do not cover (several column tiles, the fp16 numerics mode, no sorted copy).
    if (pl.modes)
        RUN(flmr_launch_s1_dense_modes(pl.scatter ? s->hit_valid : nullptr, pl.qualifying ? s->nqual : nullptr,
                                       pl.qualifying ? s->row_ovf : nullptr, c.nqueries, pl.img_rows, pl.exact_too ? 1 : 0,
                                       s->s1d_mode, s->s1d_scan_skip, s->s1d_any, st));
    if (pl.dense) {
        flmr_s1d_args d{};
        d.codes = ix->codes_sorted; d.offsets = ix->doc_offsets; d.ulen = ix->doc_ulen; d.codes_len = ix->N;
        d.idx_bits = s->idx_bits; d.idx_prefix = s->idx_prefix; d.idx_words = s->idx_words;
        d.rows = s->rows; d.row_cap = s->row_cap; d.nqual = s->nqual; d.q_lens = c.q_lens; d.nq_cand = c.nqc; d.nqueries = c.nqueries;
        d.cand = s->cand; d.cand_stride = s->cand_cap; d.cand_count = s->cand_count;
        d.band = s->s1d_band; d.band_count = s->s1d_band_count; d.mode = s->s1d_mode; d.keys = s->keys1; d.img_err = s->s1d_err; d.any = s->s1d_any;
        d.parts = 0; d.group = 64;
        RUN(flmr_launch_s1_image(d, ix->mean_ulen, st));
        RUN(flmr_launch_s1_band(s->keys1, s->cand_cap, s->cand_count, s->s1d_mode, s->s1d_err, c.nqueries, c.p.ndocs, s->s1d_band,
                                s->s1d_band_count, s->s1d_in_count, st));
        // (16 parts a query: 2 queries' rows per XCD at a time stay in its L2 -- profiles/r06/s1_dense_probe_v5.txt; groups of 16
        // candidates for a band, 32 for a whole list: the kernel's choice per query)
        d.parts = 16; d.group = 0;
        RUN(flmr_launch_s1_exact(d, ix->mean_ulen, st));
        sel_counts = s->s1d_in_count;
    }
    if (pl.recompute)   // (a query over the score-row capacity; leaves at once when there is none)
        RUN(flmr_launch_filter_stage1_recompute(c.f, s->idx_bits, s->idx_words, s->cand, s->cand_cap, s->cand_count, s->row_ovf, s->keys1,
                                                ix->centroids_f16, s->q_hi, s->q_lo, st));
    if (pl.scan)
        RUN(flmr_launch_filter_stage1(c.f, s->idx_bits, s->idx_words, s->cand, s->cand_cap, s->cand_count, s->keys1,
                                      (pl.hits && !pl.chunked) ? s->hit_bits : nullptr, s->bitmap_words, pl.hits ? s->hit_valid : nullptr,
                                      (pl.hits && pl.chunked) ? s->cand_hit : nullptr, st, (pl.modes || pl.fast) ? s->s1d_scan_skip : nullptr));
    RUN(mark(c));
    RUN(flmr_launch_select_topn(s->keys1, s->cand_cap, sel_counts, c.nqueries, c.p.ndocs, s->s1_pids, s->maxp.ndocs,
                                s->s1_count, st, out_keys, (uint64_t)ix->pid_base));
    RUN(mark(c));
    return push_status(c);
}

// S2 over s->s1_pids / s1_count -> s->keys2 (slot-aligned with s1_pids), in the full-score form of the plan
static int stage_s2(run_ctx& c) {
    flmr_searcher* s = c.s;
    const flmr_index* ix = s->ix;
    switch (c.plan.s2) {
        case s2_form::xcd:
            return flmr_launch_filter_stage2_xcd(c.f, s->s1_pids, s->maxp.ndocs, s->s1_count, c.p.ndocs, s->keys2, s->maxp.ndocs, ix,
                                                 s->q_hi, s->q_lo, s->s2_part, s->maxp.ndocs, c.st);
        case s2_form::walk:
            return flmr_launch_filter_stage2_walk(c.f, s->s1_pids, s->maxp.ndocs, s->s1_count, c.p.ndocs, s->keys2, s->maxp.ndocs,
                                                  ix->centroids_f16_tiled, s->q_hi, s->q_lo, ix->codes_sorted, c.st);
        case s2_form::gather:
            return flmr_launch_filter_stage2_mfma(c.f, s->s1_pids, s->maxp.ndocs, s->s1_count, c.p.ndocs, s->keys2, s->maxp.ndocs,
                                                  ix->centroids_f16, s->q_hi, s->q_lo, c.plan.s2_gather, c.st);
        case s2_form::gather_f32:
            return flmr_launch_filter_stage2(c.f, s->s1_pids, s->maxp.ndocs, s->s1_count, c.p.ndocs, s->keys2, s->maxp.ndocs, c.st);
        default: FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "the approximate-then-refine stage 2 runs for whole batches only");
    }
}

// S2 of a whole batch + the selection of the ndocs/4 survivors -> s->s2_pids / s2_count (in (score,pid) order, or -- approximate-
// then-refine -- as the same set)
static int stage_s2_select(run_ctx& c) {
    flmr_searcher* s = c.s;
    const flmr_index* ix = s->ix;
    const int nd4m = s->maxp.ndocs / 4;
    if (c.plan.s2 != s2_form::xcda) {
        RUN(stage_s2(c));
        return flmr_launch_sort_topn(s->keys2, s->maxp.ndocs, s->s1_count, c.p.ndocs, c.nqueries, c.p.ndocs / 4, s->s2_pids,
                                     nullptr, nd4m, s->s2_count, 0, 0, c.st);
    }
    RUN(flmr_launch_filter_stage2_xcd_ex(c.f, s->s1_pids, s->maxp.ndocs, s->s1_count, c.p.ndocs, s->keys2, s->maxp.ndocs, ix,
                                         s->q_hi, s->q_lo, s->s2_part, s->maxp.ndocs, true, c.st));
    RUN(flmr_launch_s2_refine_plan(s->keys2, s->maxp.ndocs, s->s1_count, c.p.ndocs, c.nqueries, c.p.ndocs / 4, s->q_err_sum,
                                   s->s2_pids, nd4m, s->s2_band, s->maxp.ndocs, s->s2_band_count, s->s2_need, s->s2_def, c.st));
    RUN(flmr_launch_filter_stage2_mfma(c.f, s->s2_band, s->maxp.ndocs, s->s2_band_count, c.p.ndocs, s->keys2b, s->maxp.ndocs,
                                       ix->centroids_f16, s->q_hi, s->q_lo, s2_sw::lds, c.st));
    return flmr_launch_s2_refine_finish(s->keys2b, s->maxp.ndocs, s->s2_band_count, s->s2_need, s->s2_def, c.p.ndocs, c.nqueries,
                                        s->s2_pids, nd4m, s->s2_count, c.st);
}

// S3 over s->s2_pids / s2_count -> s->keys3 / doc_scores (slot-aligned with s2_pids)
static int stage_s3(run_ctx& c, bool s0_images) {
    return flmr_launch_maxsim(s3_args(c, s0_images), c.plan.s3, c.st);
}

extern "C" int flmr_search_batch(flmr_searcher_t* s, const float* Q, const int32_t* q_lens, int32_t nqueries,
                                 int32_t nq, const flmr_search_params_t* p, int32_t* out_pids, float* out_scores,
                                 int32_t* out_counts, flmr_stream_t stream) {
    if (!out_pids || !out_scores || !out_counts) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    run_ctx c;
    RUN(prepare_ctx(c, s, Q, q_lens, nqueries, nq, p, stream, true));
    RUN(stage_s0_s1(c, nullptr));
    // ---- S2: full centroid MaxSim over the survivors, keep ndocs/4 (in (score,pid) order, or -- approximate-then-refine --
    // as the same set) ----------------
    RUN(stage_s2_select(c));
    RUN(mark(c));
    // ---- S3: decompress + normalise + MaxSim --------------------------------------------------------
    RUN(stage_s3(c, true));
    RUN(mark(c));
    // ---- S4: final ranking, global pids ---------------------------------------------------------------
    RUN(flmr_launch_sort_topn(s->keys3, s->maxp.ndocs / 4, s->s2_count, p->ndocs / 4, nqueries, p->k, out_pids,
                              out_scores, p->k, out_counts, s->ix->pid_base, 1, c.st));
    RUN(mark(c));
    if (s->profiling) {   // the set is complete: count it
        s->ev_pending++;
        s->have_ms = true;
    }
    return FLMR_OK;
}

// ---- exact sharded protocol ("exact-parity mode"): three phases with a key exchange after each --------------
// phase 1: S0..S1 on this shard -> its top-ndocs stage-1 keys (global pids), 0 padded, unordered.
extern "C" int flmr_search_phase1(flmr_searcher_t* s, const float* Q, const int32_t* q_lens, int32_t nqueries, int32_t nq,
                                  const flmr_search_params_t* p, uint64_t* out_keys, flmr_stream_t stream) {
    if (!out_keys) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    run_ctx c;
    RUN(prepare_ctx(c, s, Q, q_lens, nqueries, nq, p, stream));
    if (s->maxp.ndocs != p->ndocs) FLMR_FAIL(FLMR_ERR_INVALID, "the phased protocol needs ndocs == the searcher's max ndocs (key rows are ndocs wide)");
    return stage_s0_s1(c, out_keys);
}

// ---- query-split stage 0 (optional phase 0 of the sharded protocol) ----------------------------------------------------
// Stage 0 does not depend on the passage shard, so W ranks would repeat the same K x 128 x 32 product per query.  Instead
// rank r runs flmr_search_probe for its slice of the batch, the ranks all-gather (idx bitset, cells, ncell) -- K/8 bytes
// + a few cells per query -- and flmr_search_phase1_probed rebuilds the sparse score-table rows from the bitset.
extern "C" int flmr_searcher_probe_dims(const flmr_searcher_t* s, int32_t* idx_words, int32_t* max_cells) {
    if (!s || !idx_words || !max_cells) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    *idx_words = s->idx_words;
    *max_cells = s->max_cells;
    return FLMR_OK;
}

extern "C" int flmr_search_probe(flmr_searcher_t* s, const float* Q, const int32_t* q_lens, int32_t nqueries, int32_t nq,
                                 const flmr_search_params_t* p, int32_t q_begin, int32_t q_count, uint32_t* out_idx_bits,
                                 int32_t* out_cells, int32_t* out_ncell, flmr_stream_t stream) {
    if (q_count == 0 && s && q_begin >= 0 && q_begin <= nqueries) return FLMR_OK;  // an empty slice (more ranks than queries) has no outputs
    if (!out_idx_bits || !out_cells || !out_ncell) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    run_ctx c;
    RUN(prepare_ctx(c, s, Q, q_lens, nqueries, nq, p, stream));
    if (!c.sparse) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "query-split stage 0 needs the sparse-table path (fp16-exact centroids, K %% 64 == 0, nq_cand <= 32)");
    if (q_begin < 0 || q_count < 0 || q_begin + q_count > nqueries) FLMR_FAIL(FLMR_ERR_INVALID, "query slice [%d, %d) outside the batch of %d", q_begin, q_begin + q_count, nqueries);
    flmr_s0_args a0 = c.a0;  // the slice uses workspace slots 0..q_count; its results go straight to the caller's buffers
    a0.Q = Q + (size_t)q_begin * nq * FLMR_DIM;
    a0.q_lens = c.q_lens ? c.q_lens + q_begin : nullptr;
    a0.nqueries = q_count;
    a0.idx_bits = out_idx_bits; a0.cells = out_cells; a0.ncell = out_ncell;
    RUN(flmr_launch_centroid_scores(a0, c.plan.s0.form, c.st));
    return flmr_launch_select_cells(a0, c.st);
}

extern "C" int flmr_search_phase1_probed(flmr_searcher_t* s, const float* Q, const int32_t* q_lens, int32_t nqueries,
                                         int32_t nq, const flmr_search_params_t* p, const uint32_t* idx_bits,
                                         const int32_t* cells, const int32_t* ncell, uint64_t* out_keys,
                                         flmr_stream_t stream) {
    if (!idx_bits || !cells || !ncell || !out_keys) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    run_ctx c;
    RUN(prepare_ctx(c, s, Q, q_lens, nqueries, nq, p, stream));
    if (!c.sparse) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "query-split stage 0 needs the sparse-table path (fp16-exact centroids, K %% 64 == 0, nq_cand <= 32)");
    if (s->maxp.ndocs != p->ndocs) FLMR_FAIL(FLMR_ERR_INVALID, "the phased protocol needs ndocs == the searcher's max ndocs (key rows are ndocs wide)");
    FLMR_HIP(hipMemcpyAsync(s->idx_bits, idx_bits, (size_t)nqueries * s->idx_words * sizeof(uint32_t), hipMemcpyDeviceToDevice, c.st));
    FLMR_HIP(hipMemcpyAsync(s->cells, cells, (size_t)nqueries * s->max_cells * sizeof(int32_t), hipMemcpyDeviceToDevice, c.st));
    FLMR_HIP(hipMemcpyAsync(s->ncell, ncell, (size_t)nqueries * sizeof(int32_t), hipMemcpyDeviceToDevice, c.st));
    RUN(mark(c));
    RUN(flmr_launch_split_q(c.a0, c.st));   // (the score rows of the surviving centroids are rebuilt from the bitset by qualifying_kernel)
    RUN(mark(c));
    RUN(mark(c));
    return stage_cand_s1(c, out_keys);
}

// phase 2: global_s1 [nqueries, n_in] = the GLOBAL top-ndocs stage-1 keys; this shard scores its own members in stage 2
// -> out_keys [nqueries, ndocs], slot j = the key of global_s1[j]'s passage when it lives on this shard, else 0 (so the
// shards' outputs combine by a SUM all-reduce or by a gather).  Q / q_lens / params must be those of phase 1.
extern "C" int flmr_search_phase2(flmr_searcher_t* s, const float* Q, const int32_t* q_lens, int32_t nqueries, int32_t nq,
                                  const flmr_search_params_t* p, const uint64_t* global_s1, int32_t n_in, uint64_t* out_keys,
                                  flmr_stream_t stream) {
    if (!global_s1 || !out_keys) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    run_ctx c;
    RUN(prepare_ctx(c, s, Q, q_lens, nqueries, nq, p, stream, false, false));
    if (n_in > p->ndocs) FLMR_FAIL(FLMR_ERR_INVALID, "n_in=%d > ndocs=%d", n_in, p->ndocs);
    RUN(flmr_launch_filter_local_keys(global_s1, nqueries, n_in, s->ix->pid_base, s->ix->num_passages, s->s1_pids, s->maxp.ndocs,
                                      s->s1_count, c.st, s->s1_slot));
    RUN(stage_s2(c));
    return flmr_launch_export_keys_slotted(s->keys2, s->maxp.ndocs, s->s1_count, s->s1_slot, nqueries, (uint64_t)s->ix->pid_base,
                                           p->ndocs, out_keys, c.st);
}

// phase 3: global_s2 [nqueries, n_in] = the GLOBAL top-(ndocs/4) stage-2 keys; this shard computes the exact MaxSim of its
// own members -> out_keys [nqueries, ndocs/4], slot-aligned with global_s2 like phase 2.
extern "C" int flmr_search_phase3(flmr_searcher_t* s, const float* Q, const int32_t* q_lens, int32_t nqueries, int32_t nq,
                                  const flmr_search_params_t* p, const uint64_t* global_s2, int32_t n_in, uint64_t* out_keys,
                                  flmr_stream_t stream) {
    if (!global_s2 || !out_keys) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    run_ctx c;
    RUN(prepare_ctx(c, s, Q, q_lens, nqueries, nq, p, stream, false, false));
    if (n_in > p->ndocs / 4) FLMR_FAIL(FLMR_ERR_INVALID, "n_in=%d > ndocs/4=%d", n_in, p->ndocs / 4);
    RUN(flmr_launch_filter_local_keys(global_s2, nqueries, n_in, s->ix->pid_base, s->ix->num_passages, s->s2_pids,
                                      s->maxp.ndocs / 4, s->s2_count, c.st, s->s2_slot));
    RUN(stage_s3(c, false));
    return flmr_launch_export_keys_slotted(s->keys3, s->maxp.ndocs / 4, s->s2_count, s->s2_slot, nqueries,
                                           (uint64_t)s->ix->pid_base, p->ndocs / 4, out_keys, c.st);
}

// keys [nqueries, m] -> the n largest, descending, 0 padded (+ optional counts); m <= 8192
extern "C" int flmr_topn_keys(const uint64_t* keys, int32_t nqueries, int32_t m, int32_t n, uint64_t* out_keys,
                              int32_t* out_counts, flmr_stream_t stream) {
    if (!keys || !out_keys) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    return flmr_launch_sort_keys_topn(keys, nqueries, m, n, out_keys, out_counts, reinterpret_cast<hipStream_t>(stream));
}

// keys [nqueries, m] -> the n largest, UNORDERED, 0 padded (any m)
extern "C" int flmr_select_keys(const uint64_t* keys, int32_t nqueries, int32_t m, int32_t n, uint64_t* out_keys,
                                flmr_stream_t stream) {
    if (!keys || !out_keys) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    if (m < 1 || n < 1) FLMR_FAIL(FLMR_ERR_INVALID, "bad sizes m=%d n=%d", m, n);
    return flmr_launch_select_keys(keys, nqueries, m, n, out_keys, reinterpret_cast<hipStream_t>(stream));
}

// descending keys [nqueries, n] -> pids / scores / counts of the first k
extern "C" int flmr_unpack_keys(const uint64_t* keys, int32_t nqueries, int32_t n, int32_t k, int32_t* out_pids,
                                float* out_scores, int32_t* out_counts, flmr_stream_t stream) {
    if (!keys || !out_pids || !out_scores || !out_counts) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    return flmr_launch_unpack_keys(keys, nqueries, n, k, out_pids, out_scores, out_counts, reinterpret_cast<hipStream_t>(stream));
}
#undef RUN

extern "C" int flmr_searcher_tap(flmr_searcher_t* s, int32_t what, int32_t q, void* host_out, int64_t capacity,
                                 int64_t* count) {
    if (!s || !host_out || !count) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    if (q < 0 || q >= s->last_nqueries) FLMR_FAIL(FLMR_ERR_INVALID, "query %d outside the last batch (%d)", q, s->last_nqueries);
    FLMR_HIP(hipStreamSynchronize(s->last_stream));
    {
        const int rc = poll_status(s, true);
        if (rc) return rc;
    }
    const flmr_index* ix = s->ix;
    const flmr_plan& pl = s->last_plan;
    const void* src = nullptr;
    int64_t n = 0;
    size_t esz = 4;
    int32_t c = 0;
    const int nd4 = s->maxp.ndocs / 4;
    switch (what) {
        case FLMR_TAP_CENTROID_SCORES:
            if (pl.sparse) FLMR_FAIL(FLMR_ERR_INVALID, "the last batch ran with the sparse score table: call flmr_searcher_set_full_table(s, 1) first");
            n = (int64_t)ix->K * s->last_ncol; src = s->cs + (size_t)q * n; break;
        case FLMR_TAP_IDX_BITS:
            n = s->idx_words; src = s->idx_bits + (size_t)q * n; break;
        case FLMR_TAP_CELLS:
            FLMR_HIP(hipMemcpy(&c, s->ncell + q, 4, hipMemcpyDeviceToHost));
            n = c; src = s->cells + (size_t)q * s->max_cells; break;
        case FLMR_TAP_CANDIDATES:
            if (s->last_cand_lazy) {  // the hot path skipped the ascending lists: build them now from the bitmaps
                int rc = flmr_launch_cand_emit_all(s->last_ca, s->last_stream);
                if (rc) return rc;
                FLMR_HIP(hipStreamSynchronize(s->last_stream));
                s->last_cand_lazy = false;
            }
            FLMR_HIP(hipMemcpy(&c, s->cand_count + q, 4, hipMemcpyDeviceToHost));
            n = c; src = s->cand + (size_t)q * s->cand_cap; break;
        case FLMR_TAP_STAGE1:
            FLMR_HIP(hipMemcpy(&c, s->s1_count + q, 4, hipMemcpyDeviceToHost));
            n = c; src = s->s1_pids + (size_t)q * s->maxp.ndocs; break;
        case FLMR_TAP_STAGE2:
            FLMR_HIP(hipMemcpy(&c, s->s2_count + q, 4, hipMemcpyDeviceToHost));
            n = c; src = s->s2_pids + (size_t)q * nd4; break;
        case FLMR_TAP_DOC_SCORES:
            FLMR_HIP(hipMemcpy(&c, s->s2_count + q, 4, hipMemcpyDeviceToHost));
            n = c; src = s->doc_scores + (size_t)q * nd4; break;
        case FLMR_TAP_Q_ERR:
            n = pl.hi_first ? 32 : 0; src = s->q_err + (size_t)q * s->ncol_max; break;
        case FLMR_TAP_Q_ERR_SUM:
            n = pl.hi_first ? 1 : 0; src = s->q_err_sum + q; break;
        case FLMR_TAP_STAGE1_FORM:
            if (pl.qualifying) {   // 7: a query over the score-row capacity (stage 1 recomputed from the centroids)
                int32_t ro = 0;
                FLMR_HIP(hipMemcpy(&ro, s->row_ovf + q, 4, hipMemcpyDeviceToHost));
                if (ro) {
                    *count = 1;
                    if (capacity < 1) FLMR_FAIL(FLMR_ERR_CAPACITY, "tap needs 1 element");
                    *static_cast<int32_t*>(host_out) = 7;
                    return FLMR_OK;
                }
            }
            if (pl.dense) {   // a query the dense forms took: 5 (images + band) / 6 (exact rows)
                int32_t m = 0;
                FLMR_HIP(hipMemcpy(&m, s->s1d_mode + q, 4, hipMemcpyDeviceToHost));
                if (m != FLMR_S1D_SKIP) {
                    *count = 1;
                    if (capacity < 1) FLMR_FAIL(FLMR_ERR_CAPACITY, "tap needs 1 element");
                    *static_cast<int32_t*>(host_out) = 4 + m;
                    return FLMR_OK;
                }
            }
            n = (pl.scatter && s->last_ca.fast_state) ? 1 : 0; src = s->cand_fast + FLMR_FAST_HDR + q; break;
        default: FLMR_FAIL(FLMR_ERR_INVALID, "unknown tap %d", what);
    }
    *count = n;
    if (n > capacity) FLMR_FAIL(FLMR_ERR_CAPACITY, "tap needs %lld elements, capacity %lld", (long long)n, (long long)capacity);
    if (n) FLMR_HIP(hipMemcpy(host_out, src, (size_t)n * esz, hipMemcpyDeviceToHost));
    return FLMR_OK;
}

extern "C" int flmr_searcher_cand_bitmaps(flmr_searcher_t* s, int32_t q, int32_t* state) {
    if (!s || !state) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    if (q < 0 || q >= s->last_nqueries) FLMR_FAIL(FLMR_ERR_INVALID, "query %d outside the last batch (%d)", q, s->last_nqueries);
    FLMR_HIP(hipStreamSynchronize(s->last_stream));
    *state = -1;
    if (!(s->last_plan.scatter && s->last_ca.fast_state && s->last_ca.implied)) return FLMR_OK;
    int32_t imp = 0, word = 0, kc = 0;
    FLMR_HIP(hipMemcpy(&imp, s->cand_implied + q, 4, hipMemcpyDeviceToHost));
    FLMR_HIP(hipMemcpy(&word, s->cand_fast + FLMR_FAST_HDR + q, 4, hipMemcpyDeviceToHost));
    FLMR_HIP(hipMemcpy(&kc, s->cand_fast + FLMR_FAST_HDR + s->last_nqueries + q, 4, hipMemcpyDeviceToHost));
    *state = flmr_cand_bitmaps_state(imp, word, kc, s->last_ca.n_select);
    return FLMR_OK;
}
