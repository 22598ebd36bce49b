// Index residency: host arrays in the reference's CPU layout -> HBM (flmr_index_open / flmr_index_close).
// Replaces IndexLoader + ResidualCodec.load + ResidualEmbeddings.load_chunks (TPC/search/index_loader.py:14-86,
// TPC/indexing/codecs/residual.py:134-150, TPC/indexing/codecs/residual_embeddings.py:27-52).
#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "flmr_common.h"

thread_local char flmr_err_buf[512] = {0};

// ---- variant switches: parsed once from the environment, then changed only by flmr_set_option ----------------------------
// One entry per switch: its name, the accepted values (NULL: a set-or-unset flag, "#": an integer) and where a value lands.
struct opt_value { const char* name; int v; };
struct opt_spec { const char* name; const opt_value* values; int nvalues; };
static const opt_value kS0[] = {{"qs1", (int)s0_sw::qs1}, {"f16", (int)s0_sw::f16}, {"f16rs", (int)s0_sw::f16rs},
                                {"f32", (int)s0_sw::f32}, {"mfma", (int)s0_sw::f32}, {"valu", (int)s0_sw::valu}};
static const opt_value kS1[] = {{"scan", (int)s1_sw::scan}, {"slots", (int)s1_sw::slots}, {"image", (int)s1_sw::image}};
static const opt_value kS2[] = {{"xcda", (int)s2_sw::xcda}, {"xcd", (int)s2_sw::xcd}, {"walk", (int)s2_sw::walk}, {"lds", (int)s2_sw::lds},
#ifdef FLMR_EXPERIMENTAL_VARIANTS
                                {"regs", (int)s2_sw::regs}, {"ldsb", (int)s2_sw::ldsb},
#endif
};
static const opt_value kS3[] = {{"qs", (int)s3_sw::qs}, {"lean", (int)s3_sw::lean}, {"cw", (int)s3_sw::cw}, {"cwregs", (int)s3_sw::cwregs},
                                {"dma", (int)s3_sw::dma}, {"regs", (int)s3_sw::regs}, {"f32", (int)s3_sw::f32}};
static const opt_value kCand[] = {{"atomic", 1}, {"bitmaps", 2}};
static const opt_value kValu[] = {{"valu", 1}};
static const opt_value kInt[] = {{"#", 0}};
#define N_(a) (int)(sizeof(a) / sizeof(a[0]))
enum { O_S0, O_FULL_TABLE, O_CAND, O_NO_HITMAP, O_S1, O_S2, O_S0_STAGED, O_NO_MULTIQ, O_S3, O_SCORE, O_POISON, O_ROW_CAP, O_COUNT };
static const opt_spec kOpts[O_COUNT] = {
    {"FLMR_S0_IMPL", kS0, N_(kS0)}, {"FLMR_FULL_TABLE", nullptr, 0}, {"FLMR_CAND_IMPL", kCand, N_(kCand)}, {"FLMR_S1_NO_HITMAP", nullptr, 0},
    {"FLMR_S1_IMPL", kS1, N_(kS1)}, {"FLMR_S2_IMPL", kS2, N_(kS2)}, {"FLMR_S0_STAGED", nullptr, 0}, {"FLMR_S3_NO_MULTIQ", nullptr, 0},
    {"FLMR_S3_IMPL", kS3, N_(kS3)}, {"FLMR_SCORE_IMPL", kValu, 1}, {"FLMR_POISON", nullptr, 0}, {"FLMR_ROW_CAP", kInt, 1}};
#undef N_

static flmr_options g_opts;
static char g_env_err[O_COUNT][160];   // a value in the environment the library does not know ("" = none)
static std::once_flag g_opts_once;

// value (non-empty) -> the switch's field; FLMR_ERR_INVALID with the accepted values in `err`
static int parse_opt(int id, const char* value, flmr_options* o, char* err, size_t errlen) {
    const opt_spec& sp = kOpts[id];
    int v = 1;
    if (sp.values && sp.values[0].name[0] == '#') {
        char* end = nullptr;
        const long x = strtol(value, &end, 10);
        if (end == value || *end != 0) {
            snprintf(err, errlen, "%s=%s: expected an integer (score rows per query, 64 .. 65535)", sp.name, value);
            return FLMR_ERR_INVALID;
        }
        v = x < 64 ? 64 : x > 65535 ? 65535 : (int)x;
    } else if (sp.values) {
        int i = 0;
        while (i < sp.nvalues && strcmp(value, sp.values[i].name) != 0) i++;
        if (i == sp.nvalues) {
            int n = snprintf(err, errlen, "%s=%s: accepted values:", sp.name, value);
            for (int j = 0; j < sp.nvalues && n > 0 && (size_t)n < errlen; j++) n += snprintf(err + n, errlen - n, " %s", sp.values[j].name);
            return FLMR_ERR_INVALID;
        }
        v = sp.values[i].v;
    }
    switch (id) {
        case O_S0: o->s0 = (s0_sw)v; break;
        case O_FULL_TABLE: o->full_table = true; break;
        case O_CAND: o->cand_atomic = v == 1; o->cand_bitmaps = v == 2; break;
        case O_NO_HITMAP: o->s1_no_hitmap = true; break;
        case O_S1: o->s1 = (s1_sw)v; break;
        case O_S2: o->s2 = (s2_sw)v; break;
        case O_S0_STAGED: o->s0_staged = true; break;
        case O_NO_MULTIQ: o->s3_no_multiq = true; break;
        case O_S3: o->s3 = (s3_sw)v; break;
        case O_SCORE: o->score_valu = true; break;
        case O_POISON: o->poison = true; break;
        default: o->row_cap = v; break;
    }
    return FLMR_OK;
}

// the switch's field back to its unset state
static void clear_opt(int id, flmr_options* o) {
    flmr_options d{};
    switch (id) {
        case O_S0: o->s0 = d.s0; break;
        case O_FULL_TABLE: o->full_table = false; break;
        case O_CAND: o->cand_atomic = false; o->cand_bitmaps = false; break;
        case O_NO_HITMAP: o->s1_no_hitmap = false; break;
        case O_S1: o->s1 = d.s1; break;
        case O_S2: o->s2 = d.s2; break;
        case O_S0_STAGED: o->s0_staged = false; break;
        case O_NO_MULTIQ: o->s3_no_multiq = false; break;
        case O_S3: o->s3 = d.s3; break;
        case O_SCORE: o->score_valu = false; break;
        case O_POISON: o->poison = false; break;
        default: o->row_cap = 0; break;
    }
}

static void opts_from_env() {
    g_opts = flmr_options{};
    for (int i = 0; i < O_COUNT; i++) {
        g_env_err[i][0] = 0;
        const char* e = getenv(kOpts[i].name);
        if (e) (void)parse_opt(i, e[0] ? e : "1", &g_opts, g_env_err[i], sizeof(g_env_err[i]));
    }
}

int flmr_process_options(flmr_options* out) {
    std::call_once(g_opts_once, opts_from_env);
    for (int i = 0; i < O_COUNT; i++)
        if (g_env_err[i][0]) FLMR_FAIL(FLMR_ERR_INVALID, "environment variable %s", g_env_err[i]);
    *out = g_opts;
    return FLMR_OK;
}

// name = one of the FLMR_* switch names; value NULL or "" clears it.  Affects op-level calls at once and searchers
// created afterwards (existing searchers keep the snapshot taken at flmr_searcher_create).
extern "C" int flmr_set_option(const char* name, const char* value) {
    if (!name) FLMR_FAIL(FLMR_ERR_INVALID, "name is NULL");
    std::call_once(g_opts_once, opts_from_env);
    for (int i = 0; i < O_COUNT; i++)
        if (strcmp(name, kOpts[i].name) == 0) {
            if (!value || !value[0]) {
                clear_opt(i, &g_opts);
            } else {
                flmr_options o = g_opts;
                const int rc = parse_opt(i, value, &o, flmr_err_buf, sizeof(flmr_err_buf));
                if (rc) return rc;
                g_opts = o;
            }
            g_env_err[i][0] = 0;
            return FLMR_OK;
        }
    FLMR_FAIL(FLMR_ERR_INVALID, "unknown option %s", name);
}

extern "C" int flmr_abi_version(void) { return FLMR_ABI_VERSION; }
extern "C" const char* flmr_last_error(void) { return flmr_err_buf; }

extern "C" int flmr_device_count(int* count) {
    if (!count) FLMR_FAIL(FLMR_ERR_INVALID, "count is NULL");
    *count = 0;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        FLMR_FAIL(FLMR_ERR_HIP, "no HIP device visible (%s)", hipGetErrorString(e));
    }
    *count = n;
    return FLMR_OK;
}

// reversed_bit_map / decompression_lookup_table as ResidualCodec.__init__ builds them
// (TPC/indexing/codecs/residual.py:51-95): bit-reverse inside each nbits group; base-2^nbits digits MSB first.
void flmr_default_codec_tables(int nbits, uint8_t* rev, uint8_t* combos) {
    const int vpb = 8 / nbits, mask = (1 << nbits) - 1;
    for (int i = 0; i < 256; i++) {
        int z = 0;
        for (int g = 0; g < vpb; g++) {
            const int sh = 8 - nbits * (g + 1);
            const int x = (i >> sh) & mask;
            int y = 0;
            for (int b = 0; b < nbits; b++) y |= ((x >> b) & 1) << (nbits - 1 - b);
            z |= y << sh;
            combos[i * vpb + g] = (uint8_t)x;
        }
        rev[i] = (uint8_t)z;
    }
}

void flmr_build_wlut(int nbits, const float* bucket_weights, const uint8_t* rev, const uint8_t* combos, float* wlut) {
    const int vpb = 8 / nbits;
    for (int byte = 0; byte < 256; byte++)
        for (int l = 0; l < vpb; l++) wlut[byte * vpb + l] = bucket_weights[combos[(int)rev[byte] * vpb + l]];
}

template <typename T>
static int to_device(const T* src, size_t count, int memory, T** dst) {
    if (memory == FLMR_MEM_DEVICE) {
        *dst = const_cast<T*>(src);
        return FLMR_OK;
    }
    const size_t bytes = (count ? count : 1) * sizeof(T);
    FLMR_HIP(hipMalloc(reinterpret_cast<void**>(dst), bytes));
    if (count) FLMR_HIP(hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice));
    return FLMR_OK;
}

extern "C" int flmr_index_open(const flmr_index_desc_t* d, flmr_index_t** out) {
    if (!d || !out) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (d->dim != FLMR_DIM) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "dim=%d (this build is specialised for dim=128)", d->dim);
    if (d->nbits != 1 && d->nbits != 2 && d->nbits != 4 && d->nbits != 8)
        FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "nbits=%d", d->nbits);
    if (d->num_centroids <= 0 || d->num_embeddings < 0 || d->num_passages < 0) FLMR_FAIL(FLMR_ERR_INVALID, "negative sizes");
    if (d->num_passages + d->pid_base > 0x7fffffffLL) FLMR_FAIL(FLMR_ERR_UNSUPPORTED, "pids do not fit int32");
    if (!d->codes || !d->residuals || !d->doc_offsets || !d->ivf_pids || !d->ivf_offsets || !d->centroids ||
        !d->bucket_weights)
        FLMR_FAIL(FLMR_ERR_INVALID, "NULL array in descriptor");
    flmr_options opt;   // (FLMR_S2_IMPL=walk builds the walk's table on any index)
    int rc = flmr_process_options(&opt);
    if (rc) return rc;
    int ndev = 0;
    rc = flmr_device_count(&ndev);
    if (rc) return rc;

    flmr_index* ix = new (std::nothrow) flmr_index();
    if (!ix) FLMR_FAIL(FLMR_ERR_NOMEM, "host allocation failed");
    memset(ix, 0, sizeof(*ix));
    ix->dim = d->dim; ix->nbits = d->nbits; ix->K = d->num_centroids;
    ix->N = d->num_embeddings; ix->num_passages = d->num_passages; ix->pid_base = d->pid_base;
    ix->packed_dim = d->dim * d->nbits / 8;
    ix->owns = (d->memory == FLMR_MEM_HOST);
    if (hipGetDevice(&ix->device) != hipSuccess) {
        delete ix;
        FLMR_FAIL(FLMR_ERR_HIP, "hipGetDevice failed");
    }
    const int K = ix->K;

    // host-side metadata: IVF offsets (for the candidate-capacity bound) and the longest document
    std::vector<int64_t> ivf_off((size_t)K + 1), doc_off((size_t)ix->num_passages + 1);
    if (d->memory == FLMR_MEM_HOST) {
        memcpy(ivf_off.data(), d->ivf_offsets, sizeof(int64_t) * ((size_t)K + 1));
        memcpy(doc_off.data(), d->doc_offsets, sizeof(int64_t) * ((size_t)ix->num_passages + 1));
    } else {
        FLMR_HIP(hipMemcpy(ivf_off.data(), d->ivf_offsets, sizeof(int64_t) * ((size_t)K + 1), hipMemcpyDeviceToHost));
        FLMR_HIP(hipMemcpy(doc_off.data(), d->doc_offsets, sizeof(int64_t) * ((size_t)ix->num_passages + 1),
                           hipMemcpyDeviceToHost));
    }
    if (doc_off[ix->num_passages] != ix->N) {
        delete ix;
        FLMR_FAIL(FLMR_ERR_INVALID, "doc_offsets[-1]=%lld != num_embeddings=%lld", (long long)doc_off[ix->num_passages],
                  (long long)ix->N);
    }
    ix->max_doclen = 0;
    for (int64_t p = 0; p < ix->num_passages; p++) ix->max_doclen = std::max(ix->max_doclen, doc_off[p + 1] - doc_off[p]);
    std::vector<int64_t> lens((size_t)K);
    for (int c = 0; c < K; c++) lens[c] = ivf_off[c + 1] - ivf_off[c];
    std::sort(lens.begin(), lens.end(), [](int64_t x, int64_t y) { return x > y; });
    ix->ivf_len_prefix = new int64_t[(size_t)K + 1];
    ix->ivf_len_prefix[0] = 0;
    for (int c = 0; c < K; c++) ix->ivf_len_prefix[c + 1] = ix->ivf_len_prefix[c] + lens[c];
    const int64_t ivf_total = ivf_off[K];

#define FLMR_TRY(x)                 \
    do {                            \
        rc = (x);                   \
        if (rc) { flmr_index_close(ix); return rc; } \
    } while (0)
    FLMR_TRY(to_device(d->codes, (size_t)ix->N, d->memory, &ix->codes));
    FLMR_TRY(to_device(d->residuals, (size_t)ix->N * ix->packed_dim, d->memory, &ix->residuals));
    FLMR_TRY(to_device(d->doc_offsets, (size_t)ix->num_passages + 1, d->memory, &ix->doc_offsets));
    FLMR_TRY(to_device(d->ivf_pids, (size_t)ivf_total, d->memory, &ix->ivf_pids));
    FLMR_TRY(to_device(d->ivf_offsets, (size_t)K + 1, d->memory, &ix->ivf_offsets));
    FLMR_TRY(to_device(d->centroids, (size_t)K * FLMR_DIM, d->memory, &ix->centroids));
    FLMR_TRY(flmr_check_f16_exact(ix->centroids, (size_t)K * FLMR_DIM, &ix->centroids_f16_exact));
    FLMR_TRY(flmr_max_row_norm(ix->centroids, K, &ix->cen_norm_max));
    if (ix->centroids_f16_exact) {
        rc = hipMalloc(reinterpret_cast<void**>(&ix->centroids_f16), (size_t)K * FLMR_DIM * sizeof(_Float16)) == hipSuccess ? FLMR_OK : FLMR_ERR_NOMEM;
        if (rc) { snprintf(flmr_err_buf, sizeof(flmr_err_buf), "hipMalloc centroids_f16"); flmr_index_close(ix); return rc; }
        FLMR_TRY(flmr_convert_f16(ix->centroids, (size_t)K * FLMR_DIM, ix->centroids_f16));
    }
    FLMR_TRY(flmr_build_sorted_codes(ix));
    FLMR_TRY(flmr_build_tiled_centroids(ix, opt.s2 == s2_sw::walk));
    FLMR_TRY(flmr_build_doc_splits(ix));
    FLMR_TRY(flmr_build_chunk_table(ix->ivf_pids, ix->ivf_offsets, K, ix->num_passages, &ix->ivf_chunk_tab, &ix->nchunks));
    // fused decode table (always built on the host from the host bucket_weights)
    {
        const int vpb = 8 / ix->nbits;
        uint8_t rev[256], combos[256 * 8];
        float wl[256 * 8];
        for (int i = 0; i < (1 << ix->nbits); i++) ix->bucket_weights[i] = d->bucket_weights[i];
        flmr_default_codec_tables(ix->nbits, rev, combos);
        flmr_build_wlut(ix->nbits, ix->bucket_weights, rev, combos, wl);
        float* dw = nullptr;
        rc = to_device(wl, (size_t)256 * vpb, FLMR_MEM_HOST, &dw);
        if (rc) { flmr_index_close(ix); return rc; }
        ix->wlut = dw;
    }
    FLMR_TRY(flmr_build_s3_tables(ix));
#undef FLMR_TRY
    *out = ix;
    return FLMR_OK;
}

extern "C" int flmr_index_info(const flmr_index_t* ix, flmr_index_info_t* out) {
    if (!ix || !out) FLMR_FAIL(FLMR_ERR_INVALID, "NULL argument");
    memset(out, 0, sizeof(*out));
    const size_t K = (size_t)ix->K;
    size_t b = 256 * (8 / ix->nbits) * sizeof(float);
    if (ix->centroids_f16) b += K * FLMR_DIM * sizeof(_Float16);
    if (ix->centroids_f16_tiled) b += K * FLMR_DIM * sizeof(_Float16);
    if (ix->codes_sorted) b += ((size_t)ix->N + FLMR_CODE_PAD) * sizeof(int32_t);
    if (ix->doc_ulen) b += (size_t)ix->num_passages * sizeof(uint16_t);
    if (ix->doc_splits) b += (size_t)ix->num_passages * ix->nslices * sizeof(uint16_t);
    if (ix->ivf_chunk_tab) b += K * ((size_t)ix->nchunks + 1) * sizeof(uint32_t);
    if (ix->inv_norm) b += ((size_t)ix->N + 64) * sizeof(float);
    out->derived_bytes = (int64_t)b;
    out->max_doclen = ix->max_doclen;
    out->centroids_f16_exact = ix->centroids_f16_exact;
    out->stage2_slices = ix->nslices;
    out->xcd_round_robin = ix->xcd_round_robin;
    out->stage2_sliced = flmr_stage2_xcd_pays(ix) ? 1 : 0;
    out->passage_chunks = ix->nchunks;
    out->duplicate_permille = (int32_t)(ix->dup_share * 1000.0 + 0.5);
    return FLMR_OK;
}

extern "C" int flmr_index_close(flmr_index_t* ix) {
    if (!ix) return FLMR_OK;
    if (ix->owns) {
        (void)hipFree(ix->codes); (void)hipFree(ix->residuals); (void)hipFree(ix->doc_offsets);
        (void)hipFree(ix->ivf_pids); (void)hipFree(ix->ivf_offsets); (void)hipFree(ix->centroids);
    }
    (void)hipFree(ix->wlut);
    (void)hipFree(ix->wtab16);
    (void)hipFree(ix->inv_norm);
    (void)hipFree(ix->centroids_f16);
    (void)hipFree(ix->ivf_chunk_tab);
    (void)hipFree(ix->codes_sorted);
    (void)hipFree(ix->doc_ulen);
    (void)hipFree(ix->centroids_f16_tiled);
    (void)hipFree(ix->doc_splits);
    delete[] ix->ivf_len_prefix;
    delete ix;
    return FLMR_OK;
}
