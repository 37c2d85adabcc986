// segk_internal.h -- shared by the translation units of libsegk.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/segk.h"

#define SEGK_WS_ENTRIES (256 * 1024)      /* (row, split) partial candidates of a split-K score launch */
#define SEGK_PROF_SLOTS 256

struct segk_ctx {
    int device_id;
    int n_cu;
    char arch[64];
    // workspace of the split-K tail of the score stage: k [entries] int32, f [entries][2] float
    int32_t *ws_k;
    float *ws_f;
    unsigned long long *ws_u64;   // split full scan: (score, component) per queue entry, zero between uses
    // rows the one-product pre-filter could not decide: [0] count, [16..] row ids (grown on demand)
    int32_t *pre_queue;
    int64_t pre_cap;
    // split second stage of the pre-filter: partial candidates [row block][split][128 rows][4] and one ticket per row block
    float *sp2_part;
    int32_t *sp2_ticket;
    int64_t sp2_blocks;
    // persistent sequential chain (segk_seq_chain.hip): span maxima, control words, the sweep's utterance order
    void *chain_buf;
    size_t chain_bytes;
    double *fb_ktab;              // persistent FBGMM chain: fb_diag_const by count (diagonal components)
    int64_t fb_ktab_n;
    double fb_ktab_v0;
    int fb_ktab_D;
    double *fb_ptab;              // persistent FBGMM chain: log prior predictive of every row, and what it was computed from
    int64_t fb_ptab_n;
    unsigned long long fb_ptab_fp;     // fingerprint of the rows and the prior it was computed from (k_fb_fingerprint), and their shape
    int64_t fb_ptab_rows;
    int fb_ptab_D;
    unsigned long long *fb_fp_dev;     // [dev] the fingerprint's accumulator
    int fb_ptab_nt, fb_ptab_cov;
    double fb_ptab_k0, fb_ptab_v0;
    void *fbchain_buf;            // persistent FBGMM chain (segk_fbgmm.hip k_fb_chain): control words, the sweep's utterance order
    size_t fbchain_bytes;
    void *fbchain_lm;             // ... with a language model: the workgroups' copies of the bigram counts
    size_t fbchain_lm_bytes;
    void *fbchain_terms;          // ... the spans' predictive terms of one utterance, the exchange between the workgroups
    size_t fbchain_terms_bytes;
    // batch sampler: the block's tokens bucketed by slot (k_fbb_sort) + offsets
    int32_t *fbs_buf;
    size_t fbs_bytes;
    const void *fbb_scal_zeroed;  // segk_fbb_partials cleared these totals on the stream: the next segk_fbb_prepare need not
    const void *fbb_scal_stream;  // ... provided it is enqueued on the same stream
    int prof_launches;
    int32_t *defer_zero;          // segk_kmeans_score: queue length the chosen filter path still has to clear
    int pre_zeroed;
    int capturing;                // segk_graph_begin .. segk_graph_end
    // value hashes of the rows of the means most recently prepared (segk_kmeans_mark_duplicates)
    unsigned long long *row_hash;
    const void *row_hash_means;
    // rows bucketed by label (segk_rows_by_label): sorted row offsets [cap], per-block offsets, block bounds, small scratch
    int32_t *rb_sorted;
    int64_t rb_cap;
    int32_t *rb_koff;            // [64 * (rb_K + 1)]
    int rb_K;
    int32_t *rb_misc;            // blk_lo [68], dummy K, flags; then doubles (part_tot, scalars, terms)
    double *rb_term;             // [rb_K] per-component terms of the record metrics
    double *fc_terms;            // full-covariance span scores (segk_fullcov.hip k_fc_span_terms): [rows][K_max] Student-t logits
    int64_t fc_terms_n;          // ... doubles allocated
    double *fcb_ll;              // full-covariance batch step (k_fcb_token_ll): [token positions of the block][K_max] token likelihoods
    int64_t fcb_ll_n;            // ... doubles allocated
    double *fbi_z;               // item step of the stand-alone batch sweep (k_fbi_assign; k_fbi_assign_diag32: rows of K_max | 1): [tiles of a launch][FBI_T][K_max] logits where
    int64_t fbi_z_n;             // ... a tile's do not fit in LDS; doubles allocated (bounded: segk_fbitems.hip FBI_Z_MIB)
                                 // (k_fbi_predict / _diag32, segk_fbi_predict: the tiles of a launch over the query rows, the same bound)
    int32_t *fbt_tok;            // token step of the segmenter's acoustic-model batch sweep (k_fbt_compact): [16] tokens per local slice,
    int64_t fbt_tok_n;           // ... then [3][cap] (row, utterance, position) of the block's tokens; cap = int32 words per list
                                 // (k_fbi_orphans, the orphan pass of FBGMM.set_K: the same layout, an entry (i, i, 0) per orphan)
                                 // (segk_fbi_predict with cov_type 2: [2] the range of the query view's one cell, then new_tok and n_new [chunk] each)
    // hinted score path (segk_score_hint.hip): the filter's partial top-2 per (range, row), then the hint waves' result per row
    void *hint_part;
    size_t hint_part_bytes;
    float *pre_thr;              // band stage (segk_score_band.hip): threshold per entry of pre_queue
    int64_t pre_thr_cap;
    void *band_mask;             // its candidate masks, [ranges][queue capacity][2] x 16 bytes
    size_t band_mask_bytes;
    // hinted path feedback (segk_kmeans_hint_feedback): host-mapped word the band kernel writes, (call number << 32) | permille
    // of the call's rows the certificate could not decide; no stream command, no synchronisation
    volatile unsigned long long *miss_host;
    unsigned long long *miss_dev;
    unsigned int miss_seq;
    // delta score pass (segk_score_hint.hip): the base pass's image snapshot, its certified labels, the packed changed columns,
    // the previous call's means, the delta pass's (m1, m2) -- one allocation; valid only for the call tuple in delta_key
    void *delta_buf;
    size_t delta_bytes;
    unsigned int delta_seq;      // launches of k_delta_prep
    int delta_valid;             // the state in delta_buf / hint_part is that of the call delta_key describes
    const void *delta_key[6];    // row image, float32 rows, tile image, means, cand.k, cand.s
    int64_t delta_key_n[5];      // row0, n, n_emb, K_max, D
    // A pending prep: segk_kmeans_batch_finalize has run the delta prep for the NEXT hinted call inside k_batch_post, for the
    // tuple in delta_key and with what is recorded here; the hinted call that matches all of it skips its k_delta_prep launch.
    // The first hinted call after it consumes it, used or not: one that cannot take it over but has valid state repeats the prep
    // as a launch of its own (`redo`: k_batch_post's has refreshed the means' snapshot and moved the counters on; it left what
    // it found in spare control words).  Dropped (segk_delta_pending_drop) by every entry that can write
    // `means`, the tile images, K, cand or the delta buffer behind its back:
    //   segk_kmeans_prepare, segk_kmeans_mark_duplicates, segk_kmeans_init_stats, segk_kmeans_update_utt,
    //   segk_kmeans_sequential_sweep, segk_kmeans_add_item, segk_kmeans_del_item, segk_kmeans_clean_components,
    //   segk_kmeans_del_component, another segk_kmeans_batch_finalize, any score call but the hinted one (segk_kmeans_filter),
    //   a reallocation of the delta buffer or of hint_part (launch_delta_prep).
    int delta_pending;           // 1: as above; 2: dropped after k_batch_post ran it -- the next prep on this state repeats it
    const void *delta_pending_remap, *delta_pending_K, *delta_pending_stream;
    int delta_pending_cap, delta_pending_budget, delta_pending_seq;
    volatile int32_t *delta_host;    // host-mapped [4]: last call's mode, changed columns, packed tiles, positions the hint waves skipped
    int32_t *delta_host_dev;
    void *hint_fb;               // per-XCD shares and wave lifetimes of the matrix kernel's last launches, [3][8] floats + [3][8] uint32
    unsigned int hint_fb_launch;
    // full scan with the components in LDS (k_kmeans_brute_ls): (score, component) per queue entry, zero between uses
    unsigned long long *brute_ws;
    int64_t brute_ws_cap;
    // k-means batch finalize: the flagged tokens of a sweep beyond the kernel's LDS list, [5][flag_ovf_cap] int32
    int32_t *flag_ovf;
    int64_t flag_ovf_cap;
    // diagnostic probes of the batch sampler's tolerance modes (segk_fbb_set_probe); NULL = off
    double *probe_alpha, *probe_ll;
    int64_t probe_ll_ld;
    // optional timing of the main score launch (segk_profile_*): event pairs used round-robin
    int prof_on, prof_n, prof_kind;      // prof_on: 0 off, N: every Nth timed launch records its event pair
    unsigned int prof_calls;
    hipEvent_t prof_ev[SEGK_PROF_SLOTS][2];
    int64_t prof_rows[SEGK_PROF_SLOTS];
};

// does THIS launch record its event pair?  (segk_profile_enable(ctx, N): every Nth -- an event record between two kernels costs
// the stream ~3 us of bubble, 6.5 us per sweep around the headline kernel with N = 1)
static inline bool segk_prof_now(segk_ctx *ctx)
{
    if (!ctx->prof_on) return false;
    return (ctx->prof_calls++ % (unsigned int)ctx->prof_on) == 0u;
}


void segk_set_error(const char *fmt, ...);

// A launch-plan switch (SEGK_SCORE_HINT, SEGK_SCORE_PRE, SEGK_SCORE_B3, ...: they choose between paths with identical
// results), read at every call so that one context can be switched between calls: atoi of the variable, `dflt` when unset.
static inline int segk_env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}
// a workspace bound given in MiB (a launch-plan switch: another bound, the same results), in bytes; values below 1 mean the default
static inline size_t segk_env_mib(const char *name, int dflt_mib)
{
    const int mib = segk_env_int(name, dflt_mib);
    return (size_t)(mib > 0 ? mib : dflt_mib) << 20;
}

// Development switches that ALTER RESULTS (timing ablations, debug modes) or hand raw pointers to kernels exist only in builds
// with -DSEGK_DEV: the shipped library cannot be told through the environment to compute wrong answers.
#ifdef SEGK_DEV
static inline int segk_dev_env(const char *name) { return segk_env_int(name, 0); }
#else
static inline int segk_dev_env(const char *) { return 0; }
#endif

// segk_metrics.hip: the rows 0..n-1 bucketed by label (labels[row] in [0, K_max), anything else: not listed), every
// bucket in ascending row order -- the stable counting sort of the k-means batch statistics run over blocks of rows.
// Row q of label k inside block b: blk_lo[b] + sorted[blk_lo[b] + koff[b * (K_max + 1) + k] + q].  Buffers are owned
// by the context (valid until the next call).  K_max <= 8192.
int segk_rows_by_label(segk_ctx *ctx, const int32_t *labels, int64_t n, int K_max, const int32_t **blk_lo, int *n_blocks,
                       const int32_t **sorted, const int32_t **koff, void *stream);

#define SEGK_CHECK_HIP(expr)                                                                  \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            segk_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return SEGK_ERR_HIP;                                                              \
        }                                                                                     \
    } while (0)

#define SEGK_REQUIRE(cond, msg)                                             \
    do {                                                                    \
        if (!(cond)) {                                                      \
            segk_set_error("%s:%d: %s (%s)", __FILE__, __LINE__, msg, #cond); \
            return SEGK_ERR_ARG;                                            \
        }                                                                   \
    } while (0)

#define SEGK_LAUNCH_CHECK() SEGK_CHECK_HIP(hipGetLastError())

// Full-covariance components (segk_fbgmm.cov_type 2, segk_fullcov.hip) exist behind the entry points of the stand-alone FBGMM
// and of the unigram segmenter's launches per utterance (init_stats, update ops 0 / 1 / 2 / 4, score, pred_vector, assign,
// gibbs_items, record_metrics with urn = 0) and behind those of a unigram batch step (segk_fbb_prior_rows, _partials, _prepare,
// _score, _segment, _segment_map, _assign, _assign_map, _canonical: segk_fbb_dev.h) and behind segk_fbi_assign / segk_fbt_assign
// (the item step of the stand-alone batch sweep, the token step of the segmenter's acoustic-model batch sweep: segk_fbitems.hip);
// every other one refuses them by name.
#define SEGK_REFUSE_FULLCOV(f, who)                                                                                 \
    do {                                                                                                            \
        if ((f) && (f)->cov_type == 2) {                                                                            \
            segk_set_error("%s: full-covariance components (cov_type 2) are not supported by this entry point", who); \
            return SEGK_ERR_UNSUPPORTED;                                                                            \
        }                                                                                                           \
    } while (0)
// segk_fullcov.hip: the cov_type 2 forms of the segk_fbgmm_* entry points (arguments already checked by the caller)
int segk_fc_check(const segk_corpus *c, const segk_fbgmm *f, const char *who);
int segk_fc_init_stats(segk_ctx *ctx, const segk_corpus *c, segk_fbgmm *f, void *stream);
int segk_fc_update(const segk_corpus *c, segk_fbgmm *f, int op, int utt, int64_t item, int k, const uint8_t *boundaries, void *stream);
int segk_fc_score(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const int32_t *ids, int64_t row0, int64_t n, double *out,
                  void *stream);
int segk_fc_pred_vector(const segk_corpus *c, const segk_fbgmm *f, int64_t row, double *out, void *stream);
int segk_fc_assign(const segk_corpus *c, segk_fbgmm *f, int utt, int map_assign, double anneal_temp, const int32_t *new_tok,
                   const int32_t *n_new, const double *ustream, int64_t *ucursor, int64_t ucap, int32_t *status, void *stream);
int segk_fc_gibbs_items(const segk_corpus *c, segk_fbgmm *f, const int32_t *ids, int64_t n, int consider_unassigned,
                        double anneal_temp, const double *ustream, int64_t *ucursor, int64_t ucap, int32_t *status, void *stream,
                        int32_t *n_moved);      // n_moved != NULL: the MAP sweep of segk_fbgmm_map_items (no uniform is read)

// A workspace the context owns, grown on demand: *buf replaced by a fresh allocation of `bytes`.  Refuses during a graph capture
// (workspaces must exist before it), waits for `st` first (work in flight may still use the old block), frees the old block.
// The contents are gone.  On failure *buf is NULL.
int segk_ws_realloc(segk_ctx *ctx, void **buf, size_t bytes, hipStream_t st);
// ... when its recorded size *have (in the caller's unit: rows, bytes) is below `need`; records `need`.
template <class T, class N>
static inline int segk_ws_grow(segk_ctx *ctx, T **buf, N *have, N need, size_t bytes, hipStream_t st)
{
    if (*have >= need) return SEGK_OK;
    *have = 0;
    if (int rc = segk_ws_realloc(ctx, (void **)buf, bytes, st)) return rc;
    *have = need;
    return SEGK_OK;
}

// hipFuncAttributeMaxDynamicSharedMemorySize for `fn` on the CURRENT device, raised when `lds` exceeds 48 KB and what has been set
// there before.  The attribute is per device: a function-local static flag (rounds 1-2) skipped it for a second context on
// another GPU of the same process.  segk_occupancy: hipOccupancyMaxActiveBlocksPerMultiprocessor, cached per (device, function,
// threads, lds) the same way.
hipError_t segk_dyn_lds(const void *fn, size_t lds);
hipError_t segk_occupancy(const void *fn, int threads, size_t lds, int *wg_per_cu);

// ---------------------------------------------------------------------------------------
// Layout of the MFMA operand image of the k-means means ("tiles"), shared by the prepare
// and score kernels.  One tile = 32 components:
//   floats [g][lane][2], g < G = ceil(D/4), lane < 64:
//        M[32*tile + (lane & 31)][4*g + 2*(lane >> 5) + {0,1}]
//   (g runs to the bucket GB = segk_gmax(D) >= G, zero filled beyond D)
//   followed, at float offset GB*128, by 32 floats c[i] = -|m_i|^2 / 2   (-3e38 for rows >= K_max)
//   padded with zeros to a multiple of 1024 floats (whole 16-byte x 256-thread passes).
// ---------------------------------------------------------------------------------------
static inline __host__ __device__ int segk_G(int D) { return (D + 3) / 4; }
// k-extent bucket (in groups of 4 dims) of the score-kernel instantiation that serves
// dimension D: exact for the common embedding sizes, next larger bucket otherwise (the
// operands are zero padded to the bucket, so the surplus MFMAs add exact zeros).
#define SEGK_G_BUCKETS {1, 2, 4, 6, 8, 10, 13, 16, 20, 25, 26, 28, 32, 33, 34, 40, 50, 64, 75, 100}
static inline __host__ __device__ int segk_gmax(int D)
{
    const int b[] = SEGK_G_BUCKETS;
    int G = segk_G(D);
    for (unsigned i = 0; i < sizeof(b) / sizeof(b[0]); i++)
        if (G <= b[i]) return b[i];
    return -1;
}
// tile stride in floats: the bucket's image ([GB][64][2] operand floats + 32 constants)
// rounded up to whole 1024-float passes
static inline __host__ __device__ int segk_tile_stride(int D)
{
    int gm = segk_gmax(D);
    if (gm < 0) gm = segk_G(D);
    int f = gm * 128 + 32;
    return (f + 1023) / 1024 * 1024;
}
static inline __host__ __device__ int segk_n_tiles(int K_max) { return (K_max + 31) / 32; }

// ---------------------------------------------------------------------------------------
// Operand images of the split-precision k-means filter (float32 data, 8 <= D <= 128; segk_score_sp.hip, segk_score_h1.hip).
// fp16x2: two fp16 pieces (P = 2) of 2^a x (power-of-two scaling), the second one carried at 2^11 times its weight.
//   rows   [SEGK_SP_HEADER bytes: int32 {P, exponent a, bits of max |x_d|, 0}, int64 n_emb * KP] then P planes
//          [n_emb][KP] of 16-bit pieces (piece p of every row together), KP = D rounded up to 16 (zero padded,
//          dimensions permuted by segk_b3_dim); the float [n_emb] residual norms follow the planes
//   tiles  [1024 floats header: int32 exponent b at [0]; float E_m at [1]; [2], [3]: the batch finalize's residual
//          maximum and the exponent it built its rows with (k_batch_post reads them)] then per tile of 32 components:
//          16-bit [s][p][lane 64][8], s < KS = KP/16 (k-step), p < P (piece): piece p of
//          2^b M[32*tile + (lane & 31)][segk_b3_dim(16 s + 8 (lane >> 5) + i)], i < 8 -- the A operand of
//          v_mfma_f32_32x32x16_f16 as one 16-byte load per lane; followed, at float offset KS*P*256,
//          by 32 floats -2^(a+b) |m|^2/2 (-3e38 beyond K_max); padded to a multiple of 1024 floats.
// ---------------------------------------------------------------------------------------
#define SEGK_SP_HEADER 64
// Slot -> dimension inside a 16-wide k-step: slot q = 8h + i (h = lane half, i < 8) carries dimension
// 8 (i >> 2) + 4 h + (i & 3): each lane half owns the dimensions d with (d mod 8) in {4h .. 4h+3} of
// both 8-blocks of the step -- four complete strided accumulators of numpy's pairwise sum, so the
// winner's exact score can be finished in the score kernel without exchanging terms (the contraction
// itself is indifferent to the order of the dimensions).
static inline __host__ __device__ int segk_b3_dim(int pos)       // position in a piece row -> dimension
{
    const int q = pos & 15, h = q >> 3, i = q & 7;
    return (pos & ~15) + 8 * (i >> 2) + 4 * h + (i & 3);
}
static inline __host__ __device__ int segk_b3_kp(int D) { return (D + 15) & ~15; }
// floats per tile of P pieces (the image holds 2; segk_kmeans_tiles_b3_floats keeps the ABI's room for 3)
static inline __host__ __device__ int segk_sp_tile_stride(int D, int P)
{
    return ((segk_b3_kp(D) / 16) * P * 256 + 32 + 1023) / 1024 * 1024;
}

// segk_score_f32.hip: the MFMA score kernel in log-sum-exp mode (used by segk_fbbatch.hip); not ABI
int segk_launch_score_lse(segk_ctx *ctx, const float *Y, int64_t ldy, int D2, const int32_t *ids, int64_t row0, int64_t n,
                          const float *tiles, int n_tiles, double norm, double *out, void *stream);

// segk_prepare.hip / segk_score_sp.hip: fp16x2 images of arbitrary float32 matrices and the log-sum-exp kernel on them
int segk_sp_prepare_rows(const float *Y, int64_t ldy, int64_t n, int D2, void *img, void *stream);
int segk_sp_prepare_tiles(const float *rows, const double *consts, const double *rowmax2, int K, int D2, float *tiles_sp,
                          const void *ximg, void *stream);
int segk_launch_score_lse_sp(segk_ctx *ctx, const void *ximg, int D2, const int32_t *ids, int64_t row0, int64_t n,
                             const float *tiles_sp, int n_tiles, double norm, double *out, void *stream,
                             const int32_t *n_tiles_dev = nullptr);
int segk_launch_score_mat_sp(const void *ximg, int D2, const int32_t *ids, int64_t n, const float *tiles_sp, int n_tiles,
                             float *mat, int64_t mat_ld, void *stream, const int32_t *n_tiles_dev = nullptr, int tiles_hint = 0);
