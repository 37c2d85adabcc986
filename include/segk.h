/*
 * segk.h -- C ABI of libsegk.so: the MI355X (gfx950) implementation of the segmentalist
 * per-utterance hot path (score every candidate acoustic-word embedding against every
 * mixture component -> segmentation DP over candidate boundaries -> (re)assignment ->
 * component sufficient statistics).
 *
 * The reference (kamperh/segmentalist, Python 2 + one Cython file) has no FFI for this
 * path other than `_cython_utils.pyx`; the boundary it sits behind is a set of duck-typed
 * Python methods.  Each entry point below names the reference
 * function(s) it replaces, file:line relative to /root/reference/segmentalist/.  The
 * Python package `segmentalist_amd` binds this header with ctypes (see INTEGRATION.md for
 * the stub a maintainer of the reference would add).
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; segk_last_error() gives the text
 *     (thread local).  No exception crosses the ABI.
 *   - the CALLER owns every buffer.  Pointers marked [dev] are device (HBM) pointers,
 *     [host] are host pointers.  The library allocates nothing but the opaque segk_ctx.
 *   - `stream` is a hipStream_t passed as void*; all [dev] work is asynchronous on it.
 *   - there is NO CPU fallback: without a gfx950 device segk_create() fails.
 */
#ifndef SEGK_H
#define SEGK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEGK_OK 0
#define SEGK_ERR_ARG (-1)
#define SEGK_ERR_HIP (-2)
#define SEGK_ERR_NO_DEVICE (-3)
#define SEGK_ERR_UNSUPPORTED (-4)

#define SEGK_F32 0
#define SEGK_F64 1

typedef struct segk_ctx segk_ctx;

int32_t segk_create(int32_t device_id, segk_ctx **out_ctx);
int32_t segk_destroy(segk_ctx *ctx);
const char *segk_last_error(void);
/* ABI version, bumped on any change of a signature or of a structure below (SEGK_ABI_VERSION is the version this
 * header describes; a binding must refuse a library that reports another one: segmentalist_amd/_abi.py does).
 *   1 rounds 1-2 | 2 round 2: segk_corpus gained band_W / band_ids / band_dur (the bump was forgotten then)
 *   3 round 3: segk_fbb_set_probe, segk_kmeans_score_hinted; this check
 *   4 round 3: scratch sizes of segk_kmeans_batch_partials from segk_kmeans_batch_scratch_words; segk_profile_enable(N)
 *   5 round 3: segk_fbatch.prior_rows, segk_fbb_prior_rows
 *   6 round 4: segk_kmeans_hint_feedback; flag_rows / flag_row_bytes of the batch statistics (sharded corpus);
 *              segk_fbgmm_sequential_sweep
 *   7 round 4: segk_fbatch.consts16 holds 2 (K_max + 2) + 32 doubles (the column maps of the packed operand image behind the
 *              constants) and the token-likelihood matrix has the image's columns; the FBGMM / bigram kernels read
 *              segk_corpus.band_ids / band_dur (a COMPLETE band only); segk_fbgmm_sequential_sweep with a language model
 *   8 round 4: segk_fbb_step_diag32
 *   9 segk_fbatch.centre (the reduced-precision FBGMM kernels work in coordinates centred on it), segk_fbatch.tab32
 *  10 segk_kmeans_delta_stats
 *  11 segk_fbb_segment_map, segk_fbb_assign_map (batch sweeps with fb_type "viterbi")
 *  12 segk_fbgmm.cov_type 2 "full": the existing fields at other shapes (below); status bits 32 and 64
 *  13 cov_type 2 in the unigram segmenter's serial chain: segk_fbgmm_update op 0 and segk_fbgmm_record_metrics (urn = 0)
 *     accept it on a corpus with utterances
 *  14 cov_type 2 in the batch sampler (unigram, fp64 scores, D <= 64, K_max <= 1024, one process): segk_fbatch.partials /
 *     mean_t / q_t at other shapes (below), no structure grows; segk_fbb_prior_rows, _partials, _prepare, _score, _segment,
 * *     _segment_map, _assign, _assign_map, _canonical accept it, every other segk_fbb_* entry point keeps refusing it
 *  15 segk_fbi_assign: the item step of the stand-alone FBGMM's batch sweeps; segk_fbb_partials / _prepare / _canonical accept
 *     a corpus of items (no span tables, N_max = 1) with n_blocks = 1
 *  15 (no bump) segk_fbt_assign: the token step of the unigram segmenter's acoustic-model batch sweeps.  The rule above concerns
 *     changed signatures and structures: this adds one entry point, changes none and grows no structure, so a binding written
 *     against 15 keeps working with this library; segk_fbb_partials / _prepare accept n_blocks = 1 on a segmenter's corpus too
 *     (every token against the prior), the span-score, boundary and slot entry points keep refusing it
 *  15 (no bump) segk_fbi_assign_diag32: segk_fbi_assign for diagonal components with the Student-t terms in float32.  As for
 *     segk_fbt_assign: one entry point added, no signature or structure changed (it reads the centre / tab32 fields of 9)
 *  15 (no bump) segk_fbt_assign_diag32: segk_fbt_assign for diagonal components with the Student-t terms in float32 (the
 *     token axis of segk_fbi_assign_diag32).  Again one entry point added, no signature or structure changed
 *  15 (no bump) segk_fbi_assign_orphans: the orphan pass of FBGMM.set_K(..., sync="batch").  One entry point added, no
 *     signature or structure changed
 *  15 (no bump) segk_kmeans_batch_partials_keep + segk_kmeans_batch_keep_words: segk_kmeans_batch_partials with a caller-owned
 *     buffer through which the sums of token lists that did not change since the previous call are kept.  Two entry points
 *     added, no signature or structure changed
 *  15 (no bump) segk_fbi_assign_map, segk_fbi_assign_map_diag32, segk_fbgmm_map_items: the MAP sweeps of FBGMM.map_assign, batch
 *     and serial.  Three entry points added, no signature or structure changed
 *  15 (no bump) segk_fbi_predict, segk_fbi_predict_diag32: labels, log densities and log responsibilities of held-out rows
 *     (FBGMM.predict / score_samples / predict_log_proba).  Two entry points added, no signature or structure changed
 *  15 (no bump) segk_fbd_decode: MAP boundaries and transcript of held-out utterances (UnigramAcousticWordseg.decode).  One
 *     entry point added, no signature or structure changed
 *  15 (no bump) segk_kmd_decode: boundaries, objective and transcript of held-out utterances against a fitted segmental
 *     k-means (SegmentalKMeansWordseg.decode).  One entry point added, no signature or structure changed                   */
#define SEGK_ABI_VERSION 15
int32_t segk_abi_version(void);

/* Timing of the MAIN launch of the MFMA score kernel (k_kmeans_score<..., 0>) with HIP events
 * recorded on its launch stream inside segk_kmeans_filter (and of its log-sum-exp twin inside
 * segk_fbb_score_f32) -- what bench.py's roofline.achieved is computed from.  segk_profile_read synchronises and returns, oldest first, the duration (ms) and
 * the row count of the most recent recorded launches (at most `max`, at most 256 kept).
 * on = 0: off; on = N >= 1: every Nth timed launch records its event pair (an event record between two kernels costs the
 * stream a few microseconds of bubble: bench.py samples every 8th sweep of its timed region).                            */
int32_t segk_profile_enable(segk_ctx *ctx, int32_t on);
int32_t segk_profile_read(segk_ctx *ctx, float *ms_out, int64_t *rows_out, int32_t max);
/* Which kernel the most recent recorded launch was: 0 the fp32-MFMA filter, 2 the split-precision
 * filter (fp16x2), 1 the one-product fp16 pre-filter (k_kmeans_score_h1: rows above ~260 k,
 * D % 4 == 0), 4 the log-sum-exp kernels of the FBGMM batch sampler, 5 the range-stationary one-product
 * top-2 kernel of segk_kmeans_score_hinted (k_kmeans_top2_rs); -1 none recorded.                      */
int32_t segk_profile_last_kind(segk_ctx *ctx);
/* Number of back-to-back launches of that kernel the most recent recorded interval spans (1 since round 3 retired the
 * chunked pre-filter pipeline); the recorded duration and row count cover all of them.                            */
int32_t segk_profile_last_launches(segk_ctx *ctx);

/* hipGraph capture of a launch sequence (no reference counterpart: the reference has no device).  Every
 * kernel the library enqueues on `stream` between begin and end becomes one executable graph; segk_graph_launch replays it
 * with a single host call.  Run the sequence once before capturing it (workspaces, streams, events and
 * kernel attributes are created on first use, which a capture cannot contain); `stream` must not be the
 * legacy default stream; pointers and scalar arguments are frozen into the graph.                    */
int32_t segk_graph_begin(segk_ctx *ctx, void *stream);
int32_t segk_graph_end(segk_ctx *ctx, void *stream, void **exec_out);
int32_t segk_graph_launch(segk_ctx *ctx, void *exec, void *stream);
int32_t segk_graph_destroy(segk_ctx *ctx, void *exec);

/* -------------------------------------------------------------------------------------
 * Corpus (read-only during sampling): the device image of `Utterances` + the embedding
 * matrix (utterances.py:74-105; unigram_acoustic_wordseg.py:571-646).
 * ------------------------------------------------------------------------------------- */
typedef struct segk_corpus {
    const void *X;           /* [dev] embeddings, row-major [n_emb, ldx], dtype x_dtype      */
    const float *X32;        /* [dev] float32 image of X, row-major [n_emb, ld32] zero-padded;
                                ld32 = D rounded up to a multiple of 4.  (== X when x_dtype is
                                SEGK_F32 and ldx == ld32)                                     */
    int32_t x_dtype;         /* SEGK_F32 / SEGK_F64: dtype of X and of k-means `means`       */
    int32_t D;               /* embedding dimension                                           */
    int64_t n_emb;           /* rows of X                                                     */
    int64_t ldx;             /* leading dimension of X in elements                            */
    int64_t ld32;            /* leading dimension of X32 in floats                            */
    const float *xnorm;      /* [dev] [n_emb] upper bound of ||X[e]||_2 (segk_corpus_prepare)  */
    const int32_t *vec_ids;  /* [dev] [n_utt, tri]  span (s,t) at t(t-1)/2+s -> row of X, -1 */
    const double *durations; /* [dev] [n_utt, tri]  frames; NaN = span disallowed             */
    const int32_t *lengths;  /* [dev] [n_utt] landmarks per utterance                         */
    int32_t n_utt;
    int32_t N_max;           /* max landmarks; tri = N_max (N_max+1)/2                        */
    const void *Xb3;         /* [dev] optional (float32 data, 8 <= D <= 128): the rows split into 16-bit pieces
                                (segk_corpus_b3_bytes bytes, written by segk_corpus_prepare_b3); enables the
                                split-precision k-means filter on the 16-bit matrix pipe (NULL: fp32 MFMA)  */
    int32_t sp_pieces;       /* 2 = fp16x2: what Xb3 holds (any other value: Xb3 is not used) */
    int32_t band_W;          /* window of the banded span tables below (0: none)              */
    /* optional banded image of vec_ids / durations (utterances.py:91-105 keeps the triangular tables; the
     * per-utterance kernels only ever read the band t - s <= n_slices_max): entry (t, w), t = 1..N_max the span's
     * end, w = 0..band_W-1 its length minus one, at [(utt * N_max + t - 1) * band_W + w] = the triangular entry
     * t(t-1)/2 + (t-1-w) (-1 / NaN where that span does not exist).  Consecutive lanes read consecutive entries.
     * The k-means kernels fall back to the triangle for a span outside the band; the FBGMM / bigram kernels
     * (segk_fbgmm.hip, segk_fbbatch.hip) read the band alone when band_W equals the DP window and take it as
     * COMPLETE: pass it to them only when no triangular entry outside it names an embedding
     * (Utterances.complete_band_tables on the host side checks).                                    */
    const int32_t *band_ids; /* [dev] [n_utt, N_max, band_W] or NULL                          */
    const double *band_dur;  /* [dev] [n_utt, N_max, band_W] or NULL                          */
} segk_corpus;

/* Fill the derived members of a corpus: X32 (when X is float64 or ldx != ld32 the caller
 * passes a separate [n_emb, ld32] float buffer, written here) and xnorm. */
int32_t segk_corpus_prepare(segk_ctx *ctx, const segk_corpus *c, float *X32_out, float *xnorm_out,
                            void *stream);
/* Xb3_out [dev] segk_corpus_b3_bytes(n_emb, D) bytes (the size of three piece planes).  pieces must be 2
 * (anything else: SEGK_ERR_ARG): 2^a x = x1 + 2^-11 x2 (+ two dropped bits) in
 * fp16, a chosen from max |x|, followed -- in the room of the third plane -- by float [n_emb]
 * |x - x1| per row, which the one-product pre-filter's margin uses, and float [n_emb] -|x|^2 in the reference's
 * float32 summation order, which segk_kmeans_score_hinted uses.                                          */
int64_t segk_corpus_b3_bytes(int64_t n_emb, int32_t D);
int32_t segk_corpus_prepare_b3(segk_ctx *ctx, const segk_corpus *c, void *Xb3_out, int32_t pieces,
                               void *stream);

/* -------------------------------------------------------------------------------------
 * k-means components: device image of `KMeansComponents` (kmeans_components.py:18-91).
 * `means` has the dtype of X (kmeans_components.py:75-76: means = random_means.copy()).
 * ------------------------------------------------------------------------------------- */
typedef struct segk_kmeans {
    void *means;               /* [dev] [K_max, D] dtype x_dtype (inactive rows = random_means) */
    double *mean_numerators;   /* [dev] [K_max, D]                                              */
    int64_t *counts;           /* [dev] [K_max]                                                 */
    const void *random_means;  /* [dev] [K_max, D] dtype x_dtype                                */
    int32_t *assignments;      /* [dev] [n_emb]  component of each embedding, -1 = unassigned   */
    int32_t *K;                /* [dev] [1] number of active components                         */
    int32_t K_max;
    /* derived operands of the MFMA score kernel, maintained by the library: */
    float *tiles;              /* [dev] segk_kmeans_tiles_floats(K_max, D) floats               */
    double *mnorm_max;         /* [dev] [1] max_k ||means[k]||_2^2 (kept with atomicMax on the bits) */
    float *tiles_b3;           /* [dev] optional: segk_kmeans_tiles_b3_floats(K_max, D) floats, the fp16x2
                                  operand image of the means (maintained beside `tiles` when non-NULL) */
} segk_kmeans;

/* number of floats the caller must allocate for segk_kmeans.tiles / .tiles_b3 */
int64_t segk_kmeans_tiles_floats(int32_t K_max, int32_t D);
/* After segk_kmeans_prepare (optional; the batch sweeps call it): rows of `means` that are exact duplicates of a
 * row with a LOWER index are taken out of the filters' tile images (their accumulator seed becomes the "absent"
 * constant).  Such a row can never be np.argmax (kmeans_components.py:231: the first maximum wins, the scores are
 * bit-identical), but it turns every embedding near the pair into a tie for the full scan.  The full scan itself
 * does not read the constants.  n_marked [dev, optional]: += number of rows marked.  No-op for K_max > 2048.    */
int32_t segk_kmeans_mark_duplicates(segk_ctx *ctx, const segk_corpus *c, const segk_kmeans *m, int32_t *n_marked,
                                    void *stream);
int64_t segk_kmeans_tiles_b3_floats(int32_t K_max, int32_t D);

/* KMeansComponents.__init__ (kmeans_components.py:59-81): from `assignments` (and
 * `random_means`) build counts, mean_numerators (sequential fp64 sums in ascending row order,
 * i.e. the order of the reference's add_item loop), means, K, tiles. */
int32_t segk_kmeans_init_stats(segk_ctx *ctx, const segk_corpus *c, segk_kmeans *m, void *stream);

/* (Re)build `tiles` and `mnorm_max` from `means` (all K_max rows).  Called after any
 * wholesale change of the means. */
int32_t segk_kmeans_prepare(segk_ctx *ctx, const segk_corpus *c, segk_kmeans *m, void *stream);

/* Candidate buffers of the A1 stage, indexed by embedding row (caller-owned, n_emb entries). */
typedef struct segk_cand {
    int32_t *k;      /* [dev] [n_emb]    argmax component                                       */
    float *f;        /* [dev] [n_emb, 2] the two largest values of the fp32 filter              */
    double *s;       /* [dev] [n_emb]    max score in REFERENCE arithmetic, widened to double   */
    int32_t *queue;  /* [dev] [n_emb]    rows the filter could not decide                       */
    int32_t *count;  /* [dev] [1]        length of `queue`                                      */
} segk_cand;

/* A1 -- KMeansComponents.neg_sqrd_norm / max_ / argmax_neg_sqrd_norm_i
 * kmeans_components.py:225-232, called per embedding from get_vec_embed_neg_len_sqrd_norms
 * kmeans_acoustic_wordseg.py:334-351, for rows `ids[0..n)` (rows row0..row0+n-1 when ids == NULL;
 * entries of ids equal to -1 are skipped).  Three kernels on the stream:
 *   (1) filter: fp32 MFMA contraction of the rows of X32 against all K_max means; per row the
 *       component with the largest f[k] = x.m_k - |m_k|^2/2 and the two largest values; for
 *       float32 data with 8 <= D <= 128 the winner's score in reference arithmetic is fused in
 *       the epilogue; rows whose two best filter values are closer than the proven error
 *       margin are queued;
 *   (2) (other dtypes / D) the winner's reference-arithmetic score per row;
 *   (3) full scan of the queued rows: the reference's own computation over all K_max
 *       components, first maximum.
 * Afterwards cand->k[e] / cand->s[e] are bit-identical to np.argmax / np.max of
 * neg_sqrd_norm(e) for every processed row e (bit-exact contract).
 * status [dev] int32 [8] or NULL: status[1] accumulates the number of fully scanned rows. */
int32_t segk_kmeans_score(segk_ctx *ctx, const segk_corpus *c, const segk_kmeans *m,
                          const int32_t *ids, int64_t row0, int64_t n, const segk_cand *cand,
                          int32_t *status, void *stream);

/* segk_kmeans_score with a HINT per row (no reference counterpart; the reference recomputes every argmax from nothing,
 * kmeans_components.py:225-232): on entry cand->k[e] of every row to be processed names the component the caller expects to
 * win -- normally what the previous call left there, the row's argmax under the previous statistics -- as a label of the
 * numbering `hint_remap` translates into the current one (hint_remap [dev] int32 [K_max], e.g. the relabel table
 * segk_kmeans_batch_finalize leaves in remap_scratch; NULL = identity; values outside [0, K_max) = no hint).  The library
 * still evaluates every (row, component) product on the matrix cores, but only VERIFIES the hint against them (the two
 * largest filter values and the hinted component's reference-arithmetic score; proof in segk_score_hint.hip) instead of
 * tracking which component won; rows whose hint cannot be verified are settled among the components inside the band of the
 * filter's maximum (segk_score_band.hip; tables of more than 2048 slots: the second stage of segk_kmeans_score), what is left
 * takes the full scan.  On return cand->k /
 * cand->s are bit-identical to segk_kmeans_score's whatever the hints were: a wrong hint costs time, never correctness.
 * A segk_ctx serves one stream at a time: the path's workspaces and the per-XCD shares of its matrix kernel are the context's.
 * Applies to float32 data with the fp16x2 row image (c->Xb3, sp_pieces 2), D % 4 == 0, launches of more than 384 rows per
 * CU; everything else is forwarded to segk_kmeans_score.                                                               */
int32_t segk_kmeans_score_hinted(segk_ctx *ctx, const segk_corpus *c, const segk_kmeans *m,
                                 const int32_t *ids, int64_t row0, int64_t n, const segk_cand *cand,
                                 const int32_t *hint_remap, int32_t *status, void *stream);

/* The three steps of segk_kmeans_score as separate calls (same arguments), for callers that
 * want to time or overlap them: clear_queue (cand->count = 0), filter (kernel 1), resolve
 * (kernels 2 and 3). */
int32_t segk_kmeans_clear_queue(segk_ctx *ctx, const segk_cand *cand, void *stream);
int32_t segk_kmeans_filter(segk_ctx *ctx, const segk_corpus *c, const segk_kmeans *m,
                           const int32_t *ids, int64_t row0, int64_t n, const segk_cand *cand,
                           void *stream);
int32_t segk_kmeans_resolve(segk_ctx *ctx, const segk_corpus *c, const segk_kmeans *m,
                            const int32_t *ids, int64_t row0, int64_t n, const segk_cand *cand,
                            int32_t *status, void *stream);

/* Diagnostics of the most recent segk_kmeans_score on this context (no reference counterpart; the
 * full-size parity tests use it to prove that every stage of the path was exercised): out[0] = rows
 * the one-product pre-filter passed to its second stage (-1: the pre-filter has never run), out[1] =
 * rows in the ambiguity queue `cand->queue` (full reference-arithmetic scan).  out [host] int32 [2];
 * synchronises `stream`.                                                                          */
int32_t segk_kmeans_stage_counts(segk_ctx *ctx, const segk_cand *cand, int32_t *out, void *stream);

/* How well the hints of segk_kmeans_score_hinted are doing, WITHOUT touching any stream (no reference counterpart): hinted
 * calls on a context are numbered 1, 2, ...; *launched = number of the last one enqueued, *seen = number of the latest one
 * whose figure has reached the host (0: none yet; the device writes it into pinned host memory while the call runs),
 * *permille = thousandths of that call's rows the certificate could not decide (wrong or missing hints + near-ties).  A
 * driver that enqueues sweeps asynchronously uses it to leave the hints out (segk_kmeans_score) while most of them are
 * wrong -- the first sweeps of a chain --, where the hinted path would be the slower one; results do not depend on it.
 * launched, seen [host] uint32, permille [host] int32.                                                                  */
int32_t segk_kmeans_hint_feedback(segk_ctx *ctx, uint32_t *launched, uint32_t *seen, int32_t *permille);

/* What the delta score pass of segk_kmeans_score_hinted did, WITHOUT touching any stream (no reference counterpart; figures of
 * the latest hinted call that has reached its certificate kernel, written by the device into pinned host memory): out[0] =
 * mode, 1 delta (only the component columns whose image changed since the base pass were multiplied), 0 full, -1 the call kept
 * no delta state (SEGK_SCORE_DELTA=0, an id list, a table beyond the band stage); out[1] = image columns that differed from
 * the base pass's; out[2] = tiles of 32 packed columns multiplied (0 in full mode); out[3] = positions whose hinted score was
 * taken over from the previous call.  Results never depend on the mode.  out [host] int32 [4].                          */
int32_t segk_kmeans_delta_stats(segk_ctx *ctx, int32_t *out);

/* Gather of the A1 results for rows ids[0..n) (0..n-1 when NULL): out_max[r] (double, widened
 * from the dtype of X) and out_arg[r] = np.max / np.argmax of neg_sqrd_norm(ids[r])
 * (kmeans_components.py:228-232), from a `cand` filled by segk_kmeans_score. */
int32_t segk_kmeans_exact_max(segk_ctx *ctx, const segk_corpus *c, const segk_kmeans *m,
                              const int32_t *ids, int64_t n, const segk_cand *cand,
                              double *out_max, int32_t *out_arg, void *stream);

/* A1 full vector: out[k], k < K_max, = neg_sqrd_norm(row) in reference arithmetic; `out`
 * has the dtype of X (kmeans_components.py:169-226).                                    */
int32_t segk_kmeans_neg_sqrd_norm(segk_ctx *ctx, const segk_corpus *c, const segk_kmeans *m,
                                  int64_t row, void *out, void *stream);

/* A5 + A8 + new-segment argmax -- SegmentalKMeansWordseg.segment_i minus the statistics
 * update: get_vec_embed_neg_len_sqrd_norms (kmeans_acoustic_wordseg.py:334-351) from `cand`,
 * forward_backward_kmeans_viterbi (:449-555), get_max_unsup_transcript_i (:313,:437-446).
 * One wavefront per utterance utts[0..n_utts) (utterances utt0..utt0+n_utts-1 when utts == NULL).
 *   boundaries [dev] uint8 [n_utt, N_max]  in: current segmentation, out: new
 *   old_tok    [dev] int32 [n_utt, N_max]  embeddings of the OLD segmentation (-1 skipped)
 *   new_tok    [dev] int32 [n_utt, N_max]  embeddings of the NEW segmentation
 *   new_k      [dev] int32 [n_utt, N_max]  argmax component of each new segment
 *   n_old/n_new[dev] int32 [n_utt]
 *   n_flag     [dev] int32 [n_utt] or NULL: new segments whose argmax is an inactive row (k >= K)
 *   out_total  [dev] double [n_utt]        sum of chosen scores (:332)
 *   status     [dev] int32 [8]  [0] bit 1: a new segment has no embedding
 *              (kmeans_components.py:100 assert)                                        */
int32_t segk_kmeans_segment(segk_ctx *ctx, const segk_corpus *c, const segk_kmeans *m,
                            const int32_t *utts, int32_t utt0, int32_t n_utts,
                            int32_t n_slices_min, int32_t n_slices_max, double wip,
                            const segk_cand *cand, uint8_t *boundaries, int32_t *old_tok,
                            int32_t *new_tok, int32_t *new_k, int32_t *n_old, int32_t *n_new,
                            int32_t *n_flag, double *out_total, int32_t *status, void *stream);

/* A11 sequential update -- the tail of segment_i (kmeans_acoustic_wordseg.py:314-320):
 * del_item(old) (kmeans_components.py:113-132), add_item(new, k) (:93-111, incl. the
 * `k > K -> K` clamp), clean_components (:263-266, del_component :149-166), in exactly the
 * reference's order and floating-point arithmetic, for ONE utterance; also refreshes the
 * changed rows of `tiles` / `mnorm_max`.  Device-side, single workgroup.                */
int32_t segk_kmeans_update_utt(segk_ctx *ctx, const segk_corpus *c, segk_kmeans *m,
                               int32_t utt, const int32_t *old_tok, const int32_t *new_tok,
                               const int32_t *new_k, const int32_t *n_old, const int32_t *n_new,
                               int32_t *status, void *stream);

/* Single-item mutators with the reference's semantics (kmeans_components.py:93-166),
 * for the drop-in `KMeansComponents.add_item/del_item/del_component/clean_components`. */
int32_t segk_kmeans_add_item(segk_ctx *ctx, const segk_corpus *c, segk_kmeans *m, int64_t i,
                             int32_t k, int32_t *status, void *stream);
int32_t segk_kmeans_del_item(segk_ctx *ctx, const segk_corpus *c, segk_kmeans *m, int64_t i,
                             int32_t *status, void *stream);
int32_t segk_kmeans_clean_components(segk_ctx *ctx, const segk_corpus *c, segk_kmeans *m,
                                     int32_t *status, void *stream);

/* del_component(k) (kmeans_components.py:149-166). */
int32_t segk_kmeans_del_component(segk_ctx *ctx, const segk_corpus *c, segk_kmeans *m, int32_t k,
                                  int32_t *status, void *stream);

/* One sweep of the reference's sequential chain (SegmentalKMeansWordseg.segment's inner loop,
 * kmeans_acoustic_wordseg.py:393-399): for every utterance of `order` [HOST] int32 [n_order] in turn, segment_i
 * (:225-332) -- A1 for its spans directly in the reference's arithmetic (no filter, no operand images), the DP,
 * the del_item / add_item updates, clean_components; the operand images are refreshed once at the end.  Same
 * results as calling segk_kmeans_score / segk_kmeans_segment / segk_kmeans_update_utt per utterance (bit-identical
 * to the reference's chain).  Where the configuration allows (D % 4 = 0, 8 <= D <= 128, at most 32 landmarks per
 * utterance, 1 <= n_slices_max <= 8) the sweep runs as ONE persistent kernel (segk_seq_chain.hip: ~19 us per
 * utterance on the headline corpus); the call then synchronises `stream` after every launch of it (one launch per
 * stretch of utterances between two emptied components; not inside a graph capture).  Otherwise -- also when an
 * utterance occurs twice in `order`, which the persistent kernel's prefetch could not handle -- and with SEGK_SEQ_CHAIN=0: three launches
 * per utterance, all enqueued (~44 us per utterance).  keys_scratch [dev] uint64 [N_max (N_max + 1) / 2 + 2],
 * zeroed by the caller once.  float32 data; SEGK_ERR_UNSUPPORTED otherwise.                                   */
int32_t segk_kmeans_sequential_sweep(segk_ctx *ctx, const segk_corpus *c, segk_kmeans *m,
                                     const int32_t *order, int32_t n_order, int32_t n_slices_min,
                                     int32_t n_slices_max, double wip, const segk_cand *cand,
                                     uint64_t *keys_scratch, uint8_t *boundaries, int32_t *old_tok,
                                     int32_t *new_tok, int32_t *new_k, int32_t *n_old, int32_t *n_new,
                                     int32_t *n_flag, double *out_total, int32_t *status, void *stream);

/* A11 batch-synchronous update (DESIGN.md "batch mode"; spec: oracle/np_oracle.py
 * kmeans_batch_sweep, rank split: oracle/np_dist.py).  No reference counterpart: the reference
 * updates its statistics item by item (kmeans_components.py:93-166); the batch sweep rebuilds
 * them once per sweep in a fixed order.  Two calls, so that a multi-GPU run can exchange ONE packed
 * record per rank between them (an all-gather); `utt_lo..utt_hi` is the range of utterances owned
 * by this rank.  The sweep never touches `assignments` (all old items are deleted, all new tokens
 * added: the array is a pure function of the token lists) -- it is materialised on demand by
 * segk_kmeans_assignments_from_tokens.
 *
 * Record of one rank, in 8-byte words (nbl = n_blocks_local, FW = (2 + 3*flag_cap + 1) / 2):
 *   [part_sum nbl*K_max*D double][part_tot nbl double][part_cnt nbl*K_max int64][flags nbl*FW]
 *   flags of a block, as int32: {count, 0, (slot = utt*N_max + t, k, embedding row) x flag_cap};
 *   with flag_rows (ABI 6: a rank that holds only a SHARD of the corpus -- its own utterances' rows, numbered from 0 -- cannot
 *   read the rows of other ranks' tokens from X) followed by [rows nbl*RW], RW = (flag_cap * D * sizeof(dtype of X) + 7) / 8:
 *   the embedding rows of the block's flagged tokens themselves, in list order, which segk_kmeans_batch_finalize then reads
 *   instead of X (same values, same sums).  segk_kmeans_batch_record_words() returns the record's length
 *   (flag_row_bytes = D * sizeof(dtype of X) with flag_rows, else 0).
 *
 *  (1) segk_kmeans_batch_partials: per statistics block b (utterances [blk_lo[b], blk_lo[b+1]),
 *      blk_lo [dev] int32 [n_blocks_local + 1]) the sequential fp64 sum of its tokens per component, in
 *      token order (utterance, segment), read from the slot arrays new_tok / new_k [dev] int32
 *      [n_utt, N_max] as segk_kmeans_segment leaves them (unused slots: k = -1): a stable counting sort
 *      of the block's tokens by component (sorted_scratch: one region per (block, range of components);
 *      koff_scratch: {offset, length} of every (block, component) list; both [dev] int32, their sizes in words from
 *      segk_kmeans_batch_scratch_words -- ABI version 4; a block's regions sit at sorted_scratch + blk_lo[b] * N_max * NR
 *      words (NR = sorted_words / n_slots), so n_slots = n_utt * N_max covers any blocks, and a rank whose blocks begin at
 *      utterance u0 > 0 may allocate for n_slots = (its utterances) * N_max and pass the address of its buffer MINUS
 *      u0 * N_max * NR words: only the regions of the blocks named are touched), then one sequential sum per
 *      (block, component);
 *      part_tot = sum of out_total in utterance order.  Tokens whose argmax is an inactive row (k >= K;
 *      n_flag [dev] int32 [n_utt] counts them per utterance) are listed instead, in token order.
 *      Writes out_scalars[3] = K (before the sweep) and zeroes m->mnorm_max for (2).
 *  (2) segk_kmeans_batch_finalize: over the records of ALL ranks (records [dev], rank r at
 *      records + r * rank_stride words; n_blocks_total <= 64 blocks, n_blocks_per_rank per record):
 *      replay of the reference's `k > K -> K` clamp (kmeans_components.py:102-106) over the flagged
 *      tokens in global token order, fixed balanced-tree combination of the blocks' partial sums
 *      (components founded this sweep: sequential sums of their flagged tokens per block, same tree),
 *      means = numerators / counts, clean_components (:263-266) as a relabel table (remap_scratch [dev]
 *      int32 [K_max]), final labels of the local tokens' new_k, rebuild of the MFMA operand images
 *      (as segk_kmeans_prepare + segk_kmeans_mark_duplicates).
 *      out_scalars [dev] double [4] = {sum of totals, K, n_tokens, K before the sweep}.
 *  status bits: 1 new segment without embedding, 2 add_item on an assigned item
 *  (kmeans_components.py:101 assert), 4 more flagged tokens in one block than flag_cap (the record has room for
 *  flag_cap per block; the tokens beyond were dropped and the statistics of this sweep are NOT usable: restore a
 *  checkpoint or rebuild the state, and sweep again with a larger flag_cap.  There is no per-sweep limit).
 */
int64_t segk_kmeans_batch_record_words(int32_t K_max, int32_t D, int32_t n_blocks_local, int32_t flag_cap,
                                       int32_t flag_row_bytes);
int32_t segk_kmeans_batch_scratch_words(int32_t K_max, int64_t n_slots, int32_t n_blocks_local, int64_t *sorted_words,
                                        int64_t *koff_words);
int32_t segk_kmeans_batch_partials(segk_ctx *ctx, const segk_corpus *c, const segk_kmeans *m,
                                   const int32_t *blk_lo, int32_t n_blocks_local,
                                   const int32_t *new_tok, const int32_t *new_k, const int32_t *n_flag,
                                   const double *out_total, int32_t *sorted_scratch,
                                   int32_t *koff_scratch, double *record, int32_t flag_cap, int32_t flag_rows,
                                   double *out_scalars, void *stream);
/* segk_kmeans_batch_partials with `keep` [dev] int32 [keep_words >= segk_kmeans_batch_keep_words(K_max, n_blocks_local)], owned by
 * the caller together with sorted_scratch, koff_scratch and record, zeroed when allocated and passed to every call on those
 * three: a (block, component) list whose row ids are the ones the previous call left in sorted_scratch keeps its sum and count
 * in the record (the sum is a function of the row ids alone), every other list is summed as before -- the record is the same bit
 * for bit.  The kernel decides from a header per (block, component range) in `keep` that names the corpus, the shape and the
 * three buffers, and from the lists themselves; there is no host-side state.  Per (block b, range r) the words
 * keep[(b * NR + r) * 32 + 20 / 21] hold the lists kept / the non-empty lists summed again in the last call
 * (NR = keep_words(K_max, 1) / 32).  keep = NULL: segk_kmeans_batch_partials.  SEGK_BATCH_KEEP=0 in the environment (read per
 * call): nothing is kept.  Float64 data, odd D and D > 128 keep nothing. */
int64_t segk_kmeans_batch_keep_words(int32_t K_max, int32_t n_blocks_local);
int32_t segk_kmeans_batch_partials_keep(segk_ctx *ctx, const segk_corpus *c, const segk_kmeans *m,
                                        const int32_t *blk_lo, int32_t n_blocks_local,
                                        const int32_t *new_tok, const int32_t *new_k, const int32_t *n_flag,
                                        const double *out_total, int32_t *sorted_scratch,
                                        int32_t *koff_scratch, double *record, int32_t flag_cap, int32_t flag_rows,
                                        double *out_scalars, void *stream, int32_t *keep, int64_t keep_words);
int32_t segk_kmeans_batch_finalize(segk_ctx *ctx, const segk_corpus *c, segk_kmeans *m,
                                   int32_t utt_lo, int32_t utt_hi, const double *records,
                                   int32_t n_blocks_total, int32_t n_blocks_per_rank,
                                   int64_t rank_stride, int32_t flag_cap, int32_t flag_rows, int32_t my_rank,
                                   int32_t *new_k, int32_t *remap_scratch, double *out_scalars,
                                   int32_t *status, void *stream);
/* Record values of a batch sweep in one place (kmeans_acoustic_wordseg.py:405-420 keeps sum_neg_sqrd_norm,
 * sum_neg_len_sqrd_norm, components, n_tokens per iteration): after segk_kmeans_batch_finalize, adds
 * KMeansComponents.sum_neg_sqrd_norm (kmeans_components.py:234-247) of the tokens of utterances [utt_lo, utt_hi)
 * -- from the token lists, `assignments` is not needed -- to out_scalars[4] (zeroed by the finalize call) and copies
 * status[0], status[1] to out_scalars[5], [6]: out_scalars [dev] double [8] = {sum of totals, K, n_tokens, K before,
 * sum_neg_sqrd_norm, status bits, fully scanned rows, -}; one device-to-host copy serves the whole record.        */
int32_t segk_kmeans_batch_record(segk_ctx *ctx, const segk_corpus *c, const segk_kmeans *m, int32_t utt_lo,
                                 int32_t utt_hi, const int32_t *new_tok, const int32_t *new_k,
                                 const int32_t *status, double *out_scalars, void *stream);
/* assignments[:] = -1, then assignments[new_tok] = new_k for the tokens of utterances
 * [utt_lo, utt_hi). */
int32_t segk_kmeans_assignments_from_tokens(segk_ctx *ctx, const segk_corpus *c, segk_kmeans *m,
                                            int32_t utt_lo, int32_t utt_hi, const int32_t *new_tok,
                                            const int32_t *new_k, const int32_t *n_new,
                                            void *stream);

/* Batch refit: one Lloyd iteration over the CURRENT tokens between two batch sweeps (the reference's
 * acoustic_model.fit(m, consider_unassigned=False) of kmeans_acoustic_wordseg.py:425, kmeans.py:97-173, with the statistics
 * summed in the batch sweep's fixed order; specification: tests/kmeans_refit.py).  Entry points added at ABI 15, nothing
 * changed.  A step is: segk_kmeans_refit_collect -> segk_kmeans_score[_hinted] on the id list -> segk_kmeans_refit_apply ->
 * segk_kmeans_batch_partials -> [all-gather] -> segk_kmeans_batch_finalize, all on one stream.
 *  (1) segk_kmeans_refit_collect: the rows of the live token slots (new_k >= 0, as segk_kmeans_batch_partials reads them) of
 *      utterances [utt_lo, utt_hi) as a dense list ids [dev] int32 [n_list] in slot order, in the device's row numbering;
 *      slots [dev] int32 [n_list] or NULL: each entry's slot (utt * N_max + t); *count_out [dev] int32: the number of tokens.
 *      Entries [count, n_list) are -1 (skipped by the score calls), so the caller can score n_list entries without knowing the
 *      count: any n_list with count <= n_list <= min((utt_hi - utt_lo) * N_max, n_emb) will do; count > n_list sets status bit
 *      8 and lists the first n_list.  chunk_scratch [dev] int32 [segk_kmeans_refit_scratch_words(slots of the range)].
 *  (2) segk_kmeans_refit_apply: new_k[slot] = cand->k[row] for those tokens (np.argmax over all K_max rows), n_flag[utt] =
 *      the utterance's tokens with k >= K as segk_kmeans_segment leaves it, *moved [dev] int32 = tokens whose label changed
 *      (cleared by the call).  out_total is not touched.  A token whose row carries no result (cand->k < 0) keeps its label
 *      and sets status bit 8.  Drops the delta score pass's state: the next whole-range hinted call runs the full pass.
 *  (3) segk_kmeans_hint_relabel: cand->k[e] = table[cand->k[e]] for ALL rows e (table [dev] int32 [K_max], e.g. the
 *      finalize's remap_scratch); entries outside [0, K_max) before or after the translation become -1 = no hint, exactly what
 *      segk_kmeans_score_hinted makes of a hint and its table.  With two relabellings between a row's hint and its next use
 *      (a refit between two sweeps) the caller applies each as it happens and hints with the identity (hint_remap NULL).
 *  (4) segk_kmeans_refit_record: segk_kmeans_batch_record plus out_scalars[7] = *moved: one device-to-host copy per step.  */
int64_t segk_kmeans_refit_scratch_words(int64_t n_slots);
int32_t segk_kmeans_refit_collect(segk_ctx *ctx, const segk_corpus *c, int32_t utt_lo, int32_t utt_hi,
                                  const int32_t *new_tok, const int32_t *new_k, int32_t *chunk_scratch,
                                  int32_t *ids, int32_t *slots, int64_t n_list, int32_t *count_out,
                                  int32_t *status, void *stream);
int32_t segk_kmeans_refit_apply(segk_ctx *ctx, const segk_corpus *c, const segk_kmeans *m,
                                const segk_cand *cand, int32_t utt_lo, int32_t utt_hi,
                                const int32_t *new_tok, int32_t *new_k, int32_t *n_flag, int32_t *moved,
                                int32_t *status, void *stream);
int32_t segk_kmeans_hint_relabel(segk_ctx *ctx, const segk_corpus *c, const segk_kmeans *m,
                                 const segk_cand *cand, const int32_t *table, void *stream);
int32_t segk_kmeans_refit_record(segk_ctx *ctx, const segk_corpus *c, const segk_kmeans *m, int32_t utt_lo,
                                 int32_t utt_hi, const int32_t *new_tok, const int32_t *new_k,
                                 const int32_t *status, const int32_t *moved, double *out_scalars,
                                 void *stream);

/* KMeans.fit on the device: ONE Lloyd iteration of kmeans.py:97-173 -- the loop over the items (:113-131: np.argmax of
 * neg_sqrd_norm against the means as they stand, kmeans_components.py:225-226), the del_item / add_item of every moved item in
 * item order (kmeans.py:133-137; kmeans_components.py:93-132, add_item's clamp :101-104 included), clean_components (:263-266)
 * and the record (kmeans.py:150-153) -- enqueued by one call, with the reference's bits: assignments, means, mean_numerators,
 * counts and K are those of the item-by-item route (segk_kmeans_del_item + segk_kmeans_add_item per moved item, then
 * segk_kmeans_clean_components); specification: tests/kmeans_fit_device.py.  Entry points added at ABI 15, nothing changed.
 *   consider_unassigned != 0: every row is an item, n_items_max must be n_emb.  0: the rows with a label are (kmeans.py:118-121),
 *     listed on the device; n_items_max is any bound of their number in [1, n_emb] -- the score call runs over that many list
 *     entries, the ones behind the count are skipped; more labelled rows than n_items_max set status bit 8 (the iteration is
 *     then not usable).
 *   The number of launches does not depend on the data; the operands stay on the device.  cand->k / cand->s of the items hold
 *     np.argmax / np.max afterwards, as after segk_kmeans_score, which the call uses.  The delta score pass's state is dropped
 *     and the operand images are refreshed (segk_kmeans_prepare), as by the item-by-item route.  K_max <= 8192.
 *   scratch [dev] int32 [segk_kmeans_fit_scratch_words(n_emb, n_items_max, K_max)], contents irrelevant before and after.
 *   record [dev] double [8] = {n_mean_updates (items moved), K, items, K before, sum_neg_sqrd_norm (kmeans_components.py:234-247,
 *     tolerance-level parity as segk_kmeans_sum_neg_sqrd_norm), status[0], status[1], moves that named a row >= K}: one
 *     device-to-host copy serves the iteration's record and the early stop. */
int64_t segk_kmeans_fit_scratch_words(int64_t n_emb, int64_t n_items_max, int32_t K_max);
int32_t segk_kmeans_fit_step(segk_ctx *ctx, const segk_corpus *c, segk_kmeans *m, const segk_cand *cand,
                             int32_t consider_unassigned, int64_t n_items_max, int32_t *scratch, double *record,
                             int32_t *status, void *stream);

/* KMeansComponents.sum_neg_sqrd_norm (kmeans_components.py:234-247), record metric.
 * out [dev] double [1]; tolerance-level parity (summation order differs). */
int32_t segk_kmeans_sum_neg_sqrd_norm(segk_ctx *ctx, const segk_corpus *c, const segk_kmeans *m,
                                      double *out, void *stream);

/* -------------------------------------------------------------------------------------
 * FBGMM components: device image of `GaussianComponentsFixedVar`
 * (gaussian_components_fixedvar.py:20-126) or `GaussianComponentsDiag`
 * (gaussian_components_diag.py:19-120) plus the mixture hyper-parameters of `FBGMM`
 * (fbgmm.py:57-64).  All statistics are float64 as in the reference.
 *   cov_type 0 "fixed": prior_a = precision (1/var), prior_b = mu_0, prior_c = precision_0;
 *        stat_a = mu_N_numerators, stat_b = precision_Ns, log_prod = log_prod_precision_preds,
 *        pred = precision_preds
 *   cov_type 1 "diag":  prior_a = S_0, prior_b = m_0, (prior_c unused), k_0, v_0;
 *        stat_a = m_N_numerators, stat_b = S_N_partials, log_prod = log_prod_vars,
 *        pred = inv_vars
 *   cov_type 2 "full":  device image of `GaussianComponents` (gaussian_components.py:75-126), D <= 64, no language
 *        model.  prior_a = S_0 [D, D], prior_b = m_0 [D], k_0, v_0;
 *        stat_a = m_N_numerators [K_max, D], stat_b = S_N_partials [K_max, D, D] (row-major, symmetric),
 *        log_prod = logdet_covars [K_max], kconst as for the other types.
 *        pred [K_max, D, D] holds, where the reference keeps inv_covars, the lower Cholesky factor L of
 *        covar = (k_N + 1) / (k_N (v_N - D + 1)) (S_N_partial - k_N m_N m_N') (:319-331), recomputed from the
 *        statistics after every add and delete: pred[k][j * D + d] = L[d][j] for d >= j, 0 above the diagonal --
 *        column j of L is contiguous, it is what step j of a forward substitution reads.  logdet = 2 sum log L_dd,
 *        the Mahalanobis term of the Student-t (:334-344) is |L^-1 delta|^2.
 *        prior_c [D * D + n_emb + 1] is WRITTEN by segk_fbgmm_init_stats: the factor of the prior's covar
 *        (:207-214) in the same layout, `cached_log_prior` of every row (:125-127), and one int32 status word
 *        (in the first four bytes of the last double) for the calls that take no status argument: bit 32 = a
 *        factorisation met a non-positive or non-finite pivot (the component kept its previous factor), bit 64 =
 *        add_item / del_component named a component beyond K (nothing was done).
 *        Accepted by segk_fbgmm_init_stats, _update (ops 0, 1, 2, 4), _score, _pred_vector, _assign, _gibbs_items and
 *        _record_metrics (urn = 0) on a corpus that carries utterances (op 0 and the record are the segmenter's: on a
 *        corpus of rows alone they refuse as in ABI 12) -- with segk_unigram_segment, which never looks at the components, the launches
 *        per utterance of the unigram segmenter's serial chain.  segk_fbgmm_score evaluates lists of 16 rows or more
 *        (an utterance's triangle) a lane per row against factors staged in LDS, through a [rows, K_max] buffer of
 *        the context; shorter lists a workgroup per row.  Every other entry point that takes a segk_fbgmm returns
 *        SEGK_ERR_UNSUPPORTED: segk_fbgmm_sequential_sweep (the persistent chain kernel holds the model in LDS, and
 *        K_max D^2 doubles do not fit; the caller falls back to the launches per utterance), _update ops 5 and 6,
 *        _record_metrics with urn = 1 or on a corpus without utterances, and all of segk_fbb_* (the batch sampler).
 * ------------------------------------------------------------------------------------- */
typedef struct segk_fbgmm {
    int32_t cov_type;
    int32_t K_max;
    double alpha;              /* Dirichlet concentration (fbgmm.py:59)                       */
    double lms;                /* language-model scaling factor (fbgmm.py:62)                 */
    double k_0, v_0;           /* NIW scalars (diag only)                                     */
    const double *prior_a;     /* [dev] [D]            (full: [D, D])                         */
    const double *prior_b;     /* [dev] [D]                                                   */
    const double *prior_c;     /* [dev] [D]            (full: [D * D + n_emb + 1], derived)   */
    double *stat_a;            /* [dev] [K_max, D]                                            */
    double *stat_b;            /* [dev] [K_max, D]     (full: [K_max, D, D])                  */
    double *log_prod;          /* [dev] [K_max]                                               */
    double *pred;              /* [dev] [K_max, D]     (full: [K_max, D, D])                  */
    int64_t *counts;           /* [dev] [K_max]                                               */
    int32_t *assignments;      /* [dev] [n_emb]                                               */
    int32_t *K;                /* [dev] [1]                                                   */
    /* optional bigram language model tied to the components (BigramSmoothLM, bigram_lms.py:17-47;
     * passed to GaussianComponentsFixedVar as `lm`, gaussian_components_fixedvar.py:90): when
     * lm_unigram != NULL the assignment prior of the Dirichlet-multinomial is replaced by the LM
     * (bigram_acoustic_wordseg.py:314-384) and del_component rewires the LM counts
     * (gaussian_components_fixedvar.py:204-221). */
    int64_t *lm_unigram;       /* [dev] [K_max] or NULL                                       */
    int64_t *lm_bigram;        /* [dev] [K_max, K_max]: (j, i) = count of i following j       */
    double lm_lambda, lm_a, lm_b;
    double *kconst;            /* [dev] [K_max + 1] derived: x-independent constant of each component's
                                * predictive; entry K_max = that of the prior predictive        */
} segk_fbgmm;

/* Record metrics of one sweep on the device: out [dev] double [4] =
 *   { log_prob_z, log_prob_X_given_z, K, number of assigned rows } of the sequential-mode state in `f`:
 *   log_prob_z            FBGMM.log_prob_z, fbgmm.py:208-225 (urn = 0: Dirichlet-multinomial with f->alpha), or
 *                         BigramAcousticWordseg.log_prob_z, bigram_acoustic_wordseg.py:287-305 (urn = 1, urn_a =
 *                         lm.a: the reference's loop never advances j_prev, so it is the Polya-urn probability of
 *                         the tokens under the smoothed unigram model -- a function of the counts);
 *   log_prob_X_given_z    components.log_marg(): gaussian_components_fixedvar.py:261-296 (sums of x and x^2 per
 *                         component in the dtype of X, rows ascending, as numpy's axis-0 reduction),
 *                         gaussian_components_diag.py:271-303, or gaussian_components.py:253-303 (cov_type 2, urn = 0
 *                         only: log|S_N| and log|S_0| from the log-determinants of the factors already held).
 * Values agree with the reference's to ~1e-12 relative (contract for record values: 1e-8); workspace: the context's. */
int32_t segk_fbgmm_record_metrics(segk_ctx *ctx, const segk_corpus *c, const struct segk_fbgmm *f,
                                  int32_t urn, double urn_a, double *out, void *stream);

/* Components __init__ from `assignments` (fixedvar:110-120 / diag:114-120): statistics summed in
 * the order of the reference's add_item loop (k ascending, rows ascending), counts, K. */
int32_t segk_fbgmm_init_stats(segk_ctx *ctx, const segk_corpus *c, segk_fbgmm *f, void *stream);

/* A11 for FBGMM components, reference order and arithmetic, one workgroup:
 *   op 0: del_item for every segment of the CURRENT segmentation of utterance `utt`
 *         (unigram_acoustic_wordseg.py:270-273; boundaries [dev] uint8 [n_utt, N_max]); cov_type 2: gaussian_components.py
 *         :171-205, every delete with its refresh of the component's factor
 *   op 1: add_item(item, k)  (fixedvar:153-170 / diag:162-177)
 *   op 2: del_item(item)     (fixedvar:172-188 / diag:179-194; deletes the component when it
 *         empties: del_component fixedvar:190-221 / diag:196-213, swap-last compaction)
 *   op 4: del_component(k)
 *   op 5 / op 6: lm.remove_counts_from_utterance / lm.counts_from_utterance for the current
 *         transcript of utterance `utt` (bigram_lms.py:98-114; bigram_acoustic_wordseg.py:410,496);
 *         utt < 0: every utterance (set_lm_counts, bigram_acoustic_wordseg.py:271-276)          */
int32_t segk_fbgmm_update(segk_ctx *ctx, const segk_corpus *c, segk_fbgmm *f, int32_t op,
                          int32_t utt, int64_t item, int32_t k, const uint8_t *boundaries,
                          void *stream);

/* A2/A3/A4 -- FBGMM.log_marg_i (fbgmm.py:256-285) = logsumexp over K_max of
 * lms*(log(alpha/K_max + counts) - log(sum counts + alpha)) + log_post_pred (k < K,
 * fixedvar:242-253 / diag:237-259) or log_prior (k >= K, fixedvar:224-231 / diag:215-222), for
 * rows ids[0..n) (row0..row0+n-1 when NULL; -1 skipped); out [dev] double [n_emb] indexed by row. */
int32_t segk_fbgmm_score(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f,
                         const int32_t *ids, int64_t row0, int64_t n, double *out, void *stream);

/* A2/A3 vector API: out [dev] double [K_max + 1]: out[k] = log_post_pred(row)[k] for k < K
 * (fixedvar:242-253 / diag:237-259), out[K_max] = log_prior(row) (fixedvar:224-231 / diag:215-222). */
int32_t segk_fbgmm_pred_vector(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f,
                               int64_t row, double *out, void *stream);

/* A5 + A6/A7 for one utterance -- get_vec_embed_log_probs (unigram_acoustic_wordseg.py:474-511)
 * from the per-row scores, then forward_backward (:653-756) or forward_backward_viterbi
 * (:759-864).  Backward sampling consumes ustream[*ucursor ...] (one value per emitted segment,
 * the reference's random.random() calls) and advances the device-resident cursor.
 *   new_tok [dev] int32 [n_utt, N_max], n_new [dev] int32 [n_utt], out_logprob [dev] double [n_utt]
 *   status bits: 8 uniform stream exhausted, 16 log_prob == -inf (the reference asserts, :753)
 * viterbi == 2: `assignments_only` of bigram_acoustic_wordseg.py:386-387 -- boundaries are kept,
 * new_tok / n_new list the current segments and out_logprob[utt] = 0.                         */
int32_t segk_unigram_segment(segk_ctx *ctx, const segk_corpus *c, int32_t utt, int32_t viterbi,
                             int32_t n_slices_min, int32_t n_slices_max, double wip,
                             double time_power_term, double log_p_continue, double anneal_temp,
                             const double *score, const double *ustream, int64_t *ucursor,
                             int64_t ucap, uint8_t *boundaries, int32_t *new_tok, int32_t *n_new,
                             double *out_logprob, int32_t *status, void *stream);

/* A10 for the new segments of one utterance, in order, statistics updated between segments:
 * gibbs_sample_inside_loop_i (fbgmm.py:422-463; one uniform per segment, utils.draw forward
 * order, `k > K -> K`) or map_assign_i (:465-494) when map_assign != 0.
 * With an LM attached (f->lm_unigram != NULL): log_marg_i_embed_unigram and
 * gibbs_sample_inside_loop_i_embed (bigram_acoustic_wordseg.py:314-384): the prior of the first
 * segment is lms*lm.log_prob_vec_i(), of every later one lms*log(lm.prob_vec_given_j(k_prev)).
 * j_prev: component of the segment preceding new_tok[utt][0], -1 = none (read only with an LM). */
int32_t segk_fbgmm_assign(segk_ctx *ctx, const segk_corpus *c, segk_fbgmm *f, int32_t utt,
                          int32_t map_assign, int32_t j_prev, double anneal_temp, const int32_t *new_tok,
                          const int32_t *n_new, const double *ustream, int64_t *ucursor,
                          int64_t ucap, int32_t *status, void *stream);

/* A12: UnigramAcousticWordseg.gibbs_sample_i (unigram_acoustic_wordseg.py:252-360) for every utterance of order[0 .. n_order)
 * [host] in turn -- remove its segments, score its spans (segk_fbgmm_score), sample or maximise its boundaries
 * (segk_unigram_segment with viterbi 0 / 1), assign the new segments (segk_fbgmm_assign, map_assign) -- by ONE persistent
 * kernel per stretch of utterances between two emptied components (ABI 6): every workgroup keeps the whole model in LDS and
 * replays every update, only the span scores are shared out, one grid barrier per utterance.  Same device functions, same
 * order of operations, same uniforms (ustream / ucursor as in the per-utterance calls): the same bits as the four calls per
 * utterance.  With a language model attached (f->lm_unigram): BigramAcousticWordseg.gibbs_sample_i
 * (bigram_acoustic_wordseg.py:386-551) -- the counts of the utterance's transcript removed first and those of the new one
 * added last (segk_fbgmm_update op 5 / 6), spans scored and segments assigned under the language model; every workgroup
 * keeps its own copy of the bigram counts (K_max^2 int64 in global memory, owned by the context).
 * row_start [dev] int32 [n_utt + 1]: first row of every utterance (an utterance's rows are contiguous);
 * score [dev] double [n_emb] scratch.  Returns SEGK_ERR_UNSUPPORTED, with nothing enqueued, where the kernel does not apply
 * (more than 64 landmarks, 3 K_max D doubles beyond a workgroup's LDS, an utterance listed twice, SEGK_FB_CHAIN=0,
 * full-covariance components -- cov_type 2: K_max D^2 doubles of factors do not fit a workgroup's LDS): the
 * caller then makes the calls per utterance.  SYNCHRONISES the stream after every launch.                                  */
int32_t segk_fbgmm_sequential_sweep(segk_ctx *ctx, const segk_corpus *c, segk_fbgmm *f, const int32_t *order, int32_t n_order,
                                    const int32_t *row_start, int32_t viterbi, int32_t map_assign, int32_t n_slices_min,
                                    int32_t n_slices_max, double wip, double time_power_term, double log_p_continue,
                                    double anneal_temp_fb, double anneal_temp_am, double *score, const double *ustream,
                                    int64_t *ucursor, int64_t ucap, uint8_t *boundaries, int32_t *new_tok, int32_t *n_new,
                                    double *out_logprob, int32_t *status, void *stream);

/* Inner loop of FBGMM.gibbs_sample (fbgmm.py:352-405) over the rows ids[0..n) (ids == NULL: rows
 * 0..n-1) in order: cache_component_stats, del_item, logits (:364-372), annealing, utils.draw with
 * one uniform of the stream per considered row, then restore_component_from_stats when the row
 * went back to its component and no component was deleted, add_item otherwise.  Rows whose
 * assignment is -1 are skipped unless consider_unassigned != 0.                                */
int32_t segk_fbgmm_gibbs_items(segk_ctx *ctx, const segk_corpus *c, segk_fbgmm *f, const int32_t *ids,
                               int64_t n, int32_t consider_unassigned, double anneal_temp,
                               const double *ustream, int64_t *ucursor, int64_t ucap, int32_t *status,
                               void *stream);
/* One MAP sweep of the serial chain (added at ABI 15 without a bump; FBGMM.map_assign(sync="sequential")).  It replaces a host
 * loop over FBGMM.map_assign_i preceded by del_item: the loop of segk_fbgmm_gibbs_items (fbgmm.py:352-405) with its lines
 * 371-389 -- logits with lms, annealing, utils.draw -- replaced by map_assign_i's 475-491: z_k = log(alpha / K_max + n_k) (no
 * lms) + log predictive_k(x), k = the first maximum of exp(z - logsumexp z), then `k > K -> K`.  Per considered row in order:
 * cache_component_stats, del_item, that choice, restore_component_from_stats when the row went back to its component and no
 * component was deleted (a sweep that moves nothing leaves every statistic bit for bit), add_item otherwise.  No uniform is
 * read.  *n_moved [dev] += the rows that took the add_item branch, except a singleton that re-founded its own component (K
 * dropped by one at del_item and the row chose k == K); the caller zeroes it.  cov_type 0, 1 and 2 as segk_fbgmm_gibbs_items; a
 * language model is refused before the launch.                                                                              */
int32_t segk_fbgmm_map_items(segk_ctx *ctx, const segk_corpus *c, segk_fbgmm *f, const int32_t *ids, int64_t n,
                             int32_t consider_unassigned, int32_t *status, int32_t *n_moved, void *stream);

/* -------------------------------------------------------------------------------------
 * Batch-synchronous ("blocked parallel Gibbs") sweep of the FBGMM / bigram samplers.  The
 * reference's samplers (unigram_acoustic_wordseg.py:252-472, bigram_acoustic_wordseg.py:386-671)
 * are serial chains with no parallel mode; this family implements the sampler specified in
 * oracle/np_fbgmm_batch.py from the same building blocks: the utterances are cut into n_slices
 * contiguous slices (unit of GPU ownership and of the fixed summation order) x n_blocks blocks;
 * Gibbs step b resamples block b of every slice in parallel conditioned on all other blocks.
 * Component labels are "slots" 0..K_max-1 that are not renumbered during a sweep (count 0 = empty
 * component = prior predictive); segk_fbb_canonical gives the reference's contiguous labelling.
 * Full-covariance components (cov_type 2; specification tests/fullcov_batch.py): the calls of a unigram step with fp64
 * scores -- segk_fbb_prior_rows, _partials (needs ctx), _prepare, _score, _segment / _segment_map, _assign (ll_mat NULL) /
 * _assign_map (f32_terms 0), _canonical, with segk_fbb_collect -- take them, D <= 64, K_max <= 1024, no language model,
 * with segk_fbatch's fields at the shapes given below; _score_f32, _score_diag32, _assign_diag32, _step_diag32,
 * _token_scores, _lm_apply and _lm_fill return SEGK_ERR_UNSUPPORTED with a message that names cov_type 2, and so does any
 * call with a language model attached or D > 64.  The serial view (stat_a / stat_b / pred / log_prod / kconst / K) is not
 * written: segk_fbgmm_init_stats rebuilds it from the assignments segk_fbb_canonical leaves.
 * ------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_slices, n_blocks;   /* S (<= 16), B (>= 2)                                          */
    int32_t u_max;                /* max utterances of a (slice, block); 0 without an LM store    */
    int32_t fast_dp;              /* boundary sampler of the batch steps: 0 = fp64 library exp / log (bit-exact against the
                                   * specification), 1 = hardware v_exp_f32 / v_log_f32 (tolerance modes f32 / f16)  */
    const int32_t *utt_range;     /* [dev] [S, B, 2] utterances [lo, hi) of (slice, block)        */
    const int32_t *row_range;     /* [dev] [S, B, 2] embedding rows [lo, hi) of (slice, block)    */
    double *partials;             /* [dev] [B, S, K_max*(2D+1)]: counts [K_max] (as doubles), sum x
                                   * [K_max, D], sum x^2 [K_max, D] of the tokens of (block, slice) */
    double *cnt;                  /* [dev] [K_max]   counts of the current exclusion              */
    double *mean_t, *q_t;         /* [dev] [D, K_max] predictive mean / scale, slot-contiguous    */
    double *lconst, *zconst, *half; /* [dev] [K_max] likelihood constant, + assignment prior, multiplier */
    double *scal;                 /* [dev] [2]: total count, number of occupied slots             */
    int32_t *slot;                /* [dev] [n_emb]   slot of every embedding row, -1 = unassigned */
    int32_t *lm_tok;              /* [dev] [B, S, u_max, N_max] slots of every utterance's segments,
                                   * -1 padded (replicated on every rank); NULL without an LM     */
    uint64_t seed;                /* of the counter-based uniforms u01(seed, sweep, utt, j)       */
    /* optional fp32 matrix-core span score of fixed-variance components (segk_fbb_score_f32):      */
    float *y;                     /* [dev] [n_emb, ldy] rows [x_0^2, x_0, x_1^2, x_1, ...] (segk_fbb_make_y) */
    int64_t ldy;                  /* 2D rounded up to a multiple of 4                             */
    float *tiles32;               /* [dev] segk_kmeans_tiles_floats(K_max + 1, 2D) floats: operand
                                   * image of the per-slot [-pp/2, pp*mu] rows, written by
                                   * segk_fbb_prepare when non-NULL                               */
    /* optional fp16x2 form of the same score (2D <= 208): both operands as two fp16 pieces on the
     * 16-bit matrix pipe, like the k-means filter; needs y and, when non-NULL, supersedes tiles32:  */
    void *y16;                    /* [dev] segk_corpus_b3_bytes(n_emb, 2D) bytes (segk_fbb_make_y)  */
    float *tiles16;               /* [dev] segk_kmeans_tiles_b3_floats(K_max + 1, 2D) floats        */
    float *rows32;                /* [dev] [(K_max + 1), 2D] scratch: the per-slot rows in float32   */
    double *consts16;             /* [dev] [2 (K_max + 2) + 32] scratch: per-column constants; [K_max + 1] = max |row|^2; behind
                                     them the int32 column maps of the packed image (segk_fbb_prepare writes, the score calls read) */
    /* optional: the prior predictive of every embedding row (an empty slot's likelihood) -- a constant of corpus and prior, so
     * the score and assignment kernels of every Gibbs step need not evaluate its D logarithms per row again
     * (segk_fbb_prior_rows once; NULL: evaluated in the kernels; the values are the same either way)                           */
    const double *prior_rows;     /* [dev] [n_emb] or NULL                                         */
    /* optional: a per-dimension vector c that the reduced-precision kernels subtract from the rows and from the slot means (and
     * the prior mean) in fp64 before rounding them -- the operands of segk_fbb_make_y / segk_fbb_prepare's operand images and
     * the float32 terms of segk_fbb_score_diag32 / _assign_diag32 / _step_diag32.  Exact in real arithmetic (the densities are
     * functions of x - mu); it keeps the rounding at the data's spread instead of its distance from the origin.  Must stay
     * the same for the sampler's lifetime (segk_fbb_make_y reads it once) and on every rank.  NULL: c = 0.                    */
    const double *centre;         /* [dev] [D] or NULL                                             */
    /* optional: [dev] [2, D, K_max] floats, written by segk_fbb_prepare when non-NULL: float(mean - centre) and float(q) of
     * every slot, the tables the diagonal float32 kernels stage (each of their workgroups converted the fp64 ones itself)  */
    float *tab32;
    /* Full-covariance components (segk_fbgmm.cov_type 2): the existing fields at other shapes, as in segk_fbgmm.
     *   partials  the record of a (block, slice) cell is K_max (1 + D + D (D + 1) / 2) doubles: counts [K_max], sum x
     *             [K_max, D], the lower triangle of sum outer(x, x) per slot, packed [K_max, D (D + 1) / 2] -- entry (a, b),
     *             a >= b, at b D - b (b - 1) / 2 + (a - b); the products are rounded in the dtype of X
     *             (gaussian_components.py:116-118)
     *   mean_t    [K_max, D]     the mean m_N of every slot, slot-major
     *   q_t       [K_max, D, D]  the lower Cholesky factor of covar as segk_fbgmm.pred stores it: q_t[k][j D + d] = L[d][j]
     *   lconst    the Student-t constant of v = v_N - D + 1 degrees of freedom - logdet / 2;  half = (v + D) / 2;
     *             zconst, cnt, scal as for the other types
     * prior_rows is required; y / tiles32 / the fp16x2 buffers / centre / tab32 / lm_tok are not used.  segk_fbb_prepare sets
     * status bit 32 in the last word of segk_fbgmm.prior_c at a pivot that is not a positive finite number.             */
} segk_fbatch;

/* token lists of all utterances from the boundaries: new_tok [n_utt, N_max], n_new [n_utt]     */
int32_t segk_fbb_collect(segk_ctx *ctx, const segk_corpus *c, const uint8_t *boundaries,
                         int32_t *new_tok, int32_t *n_new, void *stream);
/* partials[b][s] for the slices s_lo .. s_lo+s_n-1 from their token lists and bt->slot: per slot
 * sequential in token order (utterance, then segment); x^2 is the square in the dtype of X
 * (gaussian_components_diag.py:125).  SIDE EFFECT: bt->scal (the totals segk_fbb_prepare accumulates into) is left
 * zeroed, so that a segk_fbb_prepare enqueued next on the same stream need not clear it; the totals are therefore only
 * valid between a segk_fbb_prepare and the next segk_fbb_partials -- call segk_fbb_prepare before reading them (or before
 * segk_fbb_score / _assign / _token_scores) after any segk_fbb_partials.  Any number of tokens per utterance (N_max > 64:
 * the lists are walked 64 tokens at a time, in order).                                                                */
int32_t segk_fbb_partials(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f,
                          const segk_fbatch *bt, int32_t s_lo, int32_t s_n, int32_t b,
                          const int32_t *new_tok, const int32_t *n_new, void *stream);
/* statistics of all tokens outside block b (b = -1: all): per slice the partials of the blocks
 * b' != b in increasing b', slices combined by the balanced tree of the specification; then the
 * predictive parameters of every slot (fixedvar:153-170,317-325 / diag:162-177,332-345).        */
int32_t segk_fbb_prepare(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f,
                         const segk_fbatch *bt, int32_t b, void *stream);
/* log_marg_i (fbgmm.py:256-285; with an LM bigram_acoustic_wordseg.py:314-329) of every row of
 * block b of the local slices under the prepared statistics -> score[row].
 * n_rows [host] [s_n]: rows of (s_lo + i, b).                                                    */
int32_t segk_fbb_score(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f,
                       const segk_fbatch *bt, int32_t s_lo, int32_t s_n, int32_t b,
                       const int32_t *n_rows, double *score, void *stream);
/* The same scores within the 1e-4 tolerance of the path, on the fp32 matrix cores (fixed-variance
 * components only): the logit of slot k is a contraction of [x^2, x] with [-pp_k/2, pp_k*mu_k] plus
 * a constant, all empty slots together are one more pseudo-component (the prior predictive, weight
 * = their number); log-sum-exp accumulated online in the MFMA kernel's epilogue.  Needs bt->y
 * (segk_fbb_make_y once) and bt->tiles32 (filled by segk_fbb_prepare).                            */
int32_t segk_fbb_make_y(segk_ctx *ctx, const segk_corpus *c, const segk_fbatch *bt, void *stream);
/* out[row] = log prior predictive of X[row] (gaussian_components_fixedvar.py:224-231 / gaussian_components_diag.py:215-222), the
 * value the score / assignment kernels use for an empty slot: for segk_fbatch.prior_rows.  Valid while X and the prior of `f`
 * stay what they are.                                                                                                          */
int32_t segk_fbb_prior_rows(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, double *out, void *stream);
int32_t segk_fbb_score_f32(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f,
                           const segk_fbatch *bt, const int32_t *rows, int64_t n, double *score,
                           void *stream);   /* rows [dev] [n]: the embedding rows to score (a block) */
/* Roofline calibration of segk_fbb_score_diag32 (no reference counterpart): Student-t terms per second of a kernel
 * that does nothing but the score kernel's inner term (subtract, multiply, multiply-add, v_log_f32, accumulate) from
 * registers on every vector ALU of the chip.  out_terms_per_s [host] double; synchronises `stream`.          */
int32_t segk_calibrate_vlog(segk_ctx *ctx, double *out_terms_per_s, void *stream);
/* segk_fbb_score for diagonal (Student-t) components in float32 with the hardware logarithm (opt-in,
 * `score_precision="f32"`): same arguments and result buffer; the reference expression is
 * gaussian_components_diag.py:237-259, 347-360 inside FBGMM.log_marg_i (fbgmm.py:256-285).  Error against the fp64
 * kernel <= 1e-4 relative to max(|log_marg_i|, 1) (the contract of the path; measured ~2e-6).                */
int32_t segk_fbb_score_diag32(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f,
                              const segk_fbatch *bt, int32_t s_lo, int32_t s_n, int32_t b,
                              const int32_t *n_rows, double *score, void *stream);
/* get_vec_embed_log_probs + forward_backward (unigram...:474-511, 653-756) for every utterance of
 * block b of the local slices with the uniforms u01(seed, sweep, utt, 0, 1, ...); the slots of the
 * old segments are cleared.  n_utts [host] [s_n].  status bit 16: log_prob == -inf.
 * Utterances of any length up to c->N_max: a corpus with N_max <= 64 keeps the utterance's span tables as triangles in LDS
 * (12 N_max (N_max + 1) / 2 bytes and a little more, at most 64 KB); a corpus with N_max > 64 keeps them as a BAND of
 * W = n_slices_max columns, the layout of c->band_ids (12 N_max W + 28 N_max + 16 + (N_max rounded up to 16) bytes of
 * the 160 KB a workgroup has), same arithmetic and same draws (N_max = 256, W = 6: 26 KB).  SEGK_ERR_ARG for such a corpus
 * when n_slices_max is 0 (unbounded) or above 64, when c has no complete band for this window (band_ids NULL or
 * band_W != n_slices_max: some span longer than the window has an embedding), or when the band does not fit.
 * With bt->fast_dp the float32 DP of the tolerance modes covers N_max <= 64 and windows <= 16; elsewhere, so for every
 * longer corpus, the fp64 recurrence runs with the hardware exponential and logarithm (inside the 1e-4 contract).   */
int32_t segk_fbb_segment(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f,
                         const segk_fbatch *bt, int32_t s_lo, int32_t s_n, int32_t b,
                         const int32_t *n_utts, uint64_t sweep, int32_t n_slices_min,
                         int32_t n_slices_max, double wip, double time_power_term,
                         double anneal_temp, const double *score, uint8_t *boundaries,
                         int32_t *new_tok, int32_t *n_new, double *out_logprob, int32_t *status,
                         void *stream);
/* slot of every new segment: softmax of the logits (fbgmm.py:436-457; with an LM
 * bigram_acoustic_wordseg.py:332-384 chained over the utterance's segments), utils.draw with
 * u01(seed, sweep, utt, N_max + position); no `k > K` clamp -- slots are drawn as such.        */
int32_t segk_fbb_assign(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f,
                        const segk_fbatch *bt, int32_t s_lo, int32_t s_n, int32_t b,
                        const int32_t *n_utts, uint64_t sweep, double anneal_temp,
                        const int32_t *new_tok, const int32_t *n_new, const float *ll_mat,
                        int64_t ll_ld, void *stream);
/* The same with the token likelihoods of diagonal (Student-t) components in float32 -- v_log_f32 terms as in
 * segk_fbb_score_diag32, z and the draws in fp64 as above (`score_precision="f32"`: log-likelihoods within 1e-4
 * relative of the fp64 form; the fp64 software logarithm of K_max * D terms per token is otherwise most of the
 * assignment step).                                                                                        */
int32_t segk_fbb_assign_diag32(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f,
                               const segk_fbatch *bt, int32_t s_lo, int32_t s_n, int32_t b,
                               const int32_t *n_utts, uint64_t sweep, double anneal_temp,
                               const int32_t *new_tok, const int32_t *n_new, void *stream);
/* Batch sweeps with fb_type "viterbi" (ABI 11): the point estimate a sampler run ends with, without leaving batch mode.
 * segk_fbb_segment_map is segk_fbb_segment with forward_backward_viterbi (unigram_acoustic_wordseg.py:759-864) in place of
 * forward_backward: a max-plus recurrence that keeps one backpointer per landmark (the candidate of the largest
 * vec + alpha, the shortest span among equal maxima: the reference's argmax(p[::-1])), and a backward pass that chases
 * them, dead ends included (:815-825).  No exponential, no logarithm, no uniform (`sweep` is accepted and ignored), no
 * temperature (the reference's Viterbi ignores it); bt->fast_dp changes nothing.  `status` is never written: a total of
 * -inf raises nothing here, as in the serial kernel, which sets bit 16 only when it samples.  Same span tables (triangles
 * for N_max <= 64, the band above), same SEGK_ERR_ARG conditions for the band, same clearing of the old segments' slots;
 * honours segk_fbb_set_probe (alpha_out receives the forward maxima).                                                     */
int32_t segk_fbb_segment_map(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f,
                             const segk_fbatch *bt, int32_t s_lo, int32_t s_n, int32_t b,
                             const int32_t *n_utts, uint64_t sweep, int32_t n_slices_min,
                             int32_t n_slices_max, double wip, double time_power_term,
                             const double *score, uint8_t *boundaries, int32_t *new_tok,
                             int32_t *n_new, double *out_logprob, int32_t *status, void *stream);
/* slot of every new segment by FBGMM.map_assign_i (fbgmm.py:465-494) on slots: the FIRST index of the maximum of
 * log(alpha / K_max + n_k) + log predictive_k(x) over all K_max slots -- no `lms` on the prior term (fbgmm.py:475-479
 * has none), no temperature, no uniform (`sweep` is accepted and ignored), no `k > K` clamp; an empty slot scores the prior
 * predictive, so all empty slots of a token tie exactly and the first one stands for them.  The token likelihoods are fp64
 * (fixed-variance: the quadratic; diagonal: the Student-t terms) or, with f32_terms != 0 (diagonal components only), the
 * float32 Student-t terms of segk_fbb_assign_diag32.  There is no ll_mat: the fp16x2 token-likelihood matrix is never
 * consumed.  SEGK_ERR_UNSUPPORTED with a language model (bigram_acoustic_wordseg.py has no Viterbi mode).  Honours
 * segk_fbb_set_probe (ll_out).                                                                                              */
int32_t segk_fbb_assign_map(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f,
                            const segk_fbatch *bt, int32_t s_lo, int32_t s_n, int32_t b,
                            const int32_t *n_utts, uint64_t sweep, const int32_t *new_tok,
                            const int32_t *n_new, int32_t f32_terms, void *stream);
/* One Gibbs step of the diagonal (Student-t) sampler in float32 terms as ONE launch (ABI 8): segk_fbb_score_diag32,
 * segk_fbb_segment and segk_fbb_assign_diag32 of block b fused -- the workgroup that owns an utterance scores its spans,
 * samples its boundaries (the same uniforms, unigram_acoustic_wordseg.py:653-864) and draws the new segments' slots from the
 * logits it already holds (fbgmm.py:422-463); `score` [dev] double [n_emb] still receives the span scores, bit for bit those
 * of segk_fbb_score_diag32, and the boundaries are those segk_fbb_segment samples from them; the token likelihoods are
 * float32 terms with one multiply-add where segk_fbb_assign_diag32 multiplies and adds (both within the 1e-4 contract).
 * Needs bt->prior_rows; honours segk_fbb_set_probe.  Returns SEGK_ERR_UNSUPPORTED, with nothing enqueued, where it does not
 * apply (a language model, K_max > 256, more than 64 landmarks per utterance, tables + logits beyond a workgroup's LDS,
 * SEGK_FBB_FUSED=0): the caller then makes the three calls.                                                                                                        */
int32_t segk_fbb_step_diag32(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt,
                             int32_t s_lo, int32_t s_n, int32_t b, const int32_t *n_utts, uint64_t sweep,
                             int32_t n_slices_min, int32_t n_slices_max, double wip, double time_power_term,
                             double anneal_temp_fb, double anneal_temp_am, double *score, uint8_t *boundaries,
                             int32_t *new_tok, int32_t *n_new, double *out_logprob, int32_t *status, void *stream);
/* ll_mat of segk_fbb_assign (optional; fixed-variance components with the fp16x2 images): the token
 * likelihoods come from the matrix-core contraction instead of the fp64 VALU loop.  Row j*N_max + t of
 * ll_mat [n, ll_ld] belongs to segment t of the j-th utterance of the block (local slices in order);
 * segk_fbb_token_scores fills it for the row list tok_rows[j*N_max + t] = new_tok[utt_j][t].  The columns
 * are those of the packed operand image of the step's segk_fbb_prepare (occupied slots in slot order, then the
 * pseudo-component of the empty ones), which segk_fbb_assign of the same step resolves; not a per-slot table. */
int32_t segk_fbb_token_scores(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f,
                              const segk_fbatch *bt, const int32_t *tok_rows, int64_t n,
                              float *ll_mat, int64_t ll_ld, void *stream);
/* Diagnostic probes of the tolerance modes (no reference counterpart; used by the parity tests to hold the float32 /
 * fp16 token likelihoods and the hardware-exp/log forward filter to the 1e-4 contract directly, not through the draws
 * they feed).  While set, on this context:
 *   segk_fbb_segment also writes the forward filter's alpha[t] (unigram_acoustic_wordseg.py:691-703), t < N, of every
 *     utterance it samples to alpha_out[utt * N_max + t]                     (alpha_out [dev] double [n_utt, N_max]);
 *   segk_fbb_assign / segk_fbb_assign_diag32 / segk_fbb_assign_map also write, for token t of utterance utt and every slot k < K_max, the
 *     log predictive density of the token under slot k that enters its logits (posterior predictive of an occupied
 *     slot, prior predictive of an empty one: oracle/np_fbgmm_batch.py `loglik`) to
 *     ll_out[(utt * N_max + t) * ll_ld + k]                                 (ll_out [dev] double [n_utt * N_max, ll_ld]).
 * NULL pointers (the default) switch a probe off.                                                                  */
int32_t segk_fbb_set_probe(segk_ctx *ctx, double *alpha_out, double *ll_out, int64_t ll_ld);
/* Batch Gibbs sweeps of the STAND-ALONE mixture model (ABI 15; FBGMM.gibbs_sample, fbgmm.py:288-463, as the blocked sampler
 * above with "utterance" read as "item"; specification tests/fbgmm_items.py).  The items are presented as a corpus of
 * one-landmark utterances: segk_corpus with n_utt = n_emb, N_max = 1 and NO span tables (vec_ids, durations, lengths,
 * band_* NULL), new_tok[i] = i, n_new[i] = 1 where item i holds a slot and 0 where it does not; bt->utt_range holds the item
 * ranges of the (slice, block) cells (bt->row_range the same numbers), bt->prior_rows is required.  The statistics are the
 * segmenter's: segk_fbb_partials, segk_fbb_prepare(b), and segk_fbb_prepare(-1) + segk_fbb_canonical + segk_fbgmm_init_stats
 * for the reference's view; on such a corpus they also take n_blocks = 1 (every item against the prior).
 * This call is step b's item half, after segk_fbb_prepare(b) and before segk_fbb_partials(b): every considered item i of block
 * b of the local slices [s_lo, s_lo + s_n) -- bt->slot[i] >= 0, or every item when consider_unassigned -- forms
 * z_k = lms log(alpha / K_max + n_k) + log predictive_k(X[i]) over all K_max slots (fbgmm.py:436-440; an empty slot: the prior
 * predictive), anneals it when anneal_temp != 1 (fbgmm.py:446-449), and draws its slot by the batch sampler's inverse-CDF walk
 * on u01(bt->seed, sweep, i, 1) -- counter N_max + t of a one-landmark utterance, so the draws are those of segk_fbb_assign on
 * the same rows as utterances.  bt->slot[i] and n_new[i] = 1 are written; an item not considered keeps -1 and 0.
 * n_items [host] [s_n]: items of block b per local slice (the widths of bt->utt_range).  cov_type 0, 1 (D <= 256) and 2
 * (D <= 64, K_max <= 1024; the likelihoods by the token-likelihood kernel of segk_fbb_assign); X float32 or float64; fp64
 * arithmetic.  A language model (f->lm_unigram) is SEGK_ERR_UNSUPPORTED.  probe_ll (NULL in production) receives the likelihood
 * part of the logits, probe_ll[i * probe_ld + k], k < K_max <= probe_ld, of every item of the block's tiles -- the role
 * segk_fbb_set_probe plays for the segmenter.  One launch per 64 items x all slots; the logits of a tile live in LDS or, beyond
 * a workgroup's budget, in a workspace of the context bounded by 64 MiB (a block of more tiles is walked in several launches).  */
int32_t segk_fbi_assign(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt,
                        int32_t s_lo, int32_t s_n, int32_t b, const int32_t *n_items, uint64_t sweep,
                        double anneal_temp, int32_t consider_unassigned, const int32_t *new_tok,
                        int32_t *n_new, double *probe_ll, int64_t probe_ld, void *stream);
/* segk_fbi_assign for diagonal components (cov_type 1) with float32 item likelihoods (added at ABI 15 without a bump;
 * FBGMM(..., sync="batch", score_precision="f32")): the same arguments, the same role in a step, the same slots written.
 * Only the likelihood half differs.  Per (item, slot) the Student-t terms are those of segk_fbb_assign_diag32 /
 * segk_fbb_step_diag32: m = float(mean - centre) and q = float(q) from bt->tab32 (segk_fbb_prepare(b) writes it when the
 * pointer is set), x = float(X[i][d] - centre[d]) with the difference formed in fp64, acc += log2(1 + (m - x)^2 q) on the
 * hardware logarithm, dimensions ascending, then ll = lconst - half * (ln 2 * acc) in fp64.  An empty slot keeps
 * bt->prior_rows[i] (fp64).  The prior's term, the softmax, the annealing and the inverse-CDF walk are segk_fbi_assign's, in
 * fp64 on these logits: the draws are the fp64 function of likelihoods that lie within the tolerance contract of the float32
 * modes (1e-4 max(|ll|, 1)) of segk_fbi_assign's.  The statistics stay fp64 and exact.
 * Refused before any launch: cov_type 0 or 2 and a language model with SEGK_ERR_UNSUPPORTED; bt->tab32, bt->centre or
 * bt->prior_rows NULL, D > 256 or a corpus with span tables with SEGK_ERR_ARG.  probe_ll as for segk_fbi_assign, the rows of the considered items only (an
 * unassigned item that is not considered leaves its row as it was).  One launch per
 * 64 items x all slots; the rows and 32 slots' tables are staged as float32 (516 D bytes of LDS), a tile's logits are 64 rows of
 * K_max | 1 doubles, in LDS where both fit in 144 KiB, else in the bounded workspace of segk_fbi_assign (SEGK_FBI_Z_MIB).        */
int32_t segk_fbi_assign_diag32(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt,
                               int32_t s_lo, int32_t s_n, int32_t b, const int32_t *n_items, uint64_t sweep,
                               double anneal_temp, int32_t consider_unassigned, const int32_t *new_tok,
                               int32_t *n_new, double *probe_ll, int64_t probe_ld, void *stream);
/* The item half of a step of a MAP sweep of the stand-alone mixture model (added at ABI 15 without a bump;
 * FBGMM.map_assign(sync="batch"); specification tests/fbgmm_items_map.py).  It stands where segk_fbi_assign stands in a step
 * -- after segk_fbb_prepare(b), before segk_fbb_partials(b) -- and replaces its draw (fbgmm.py:436-460) by the hard assignment
 * of FBGMM.map_assign_i (fbgmm.py:465-494) on slots: every considered item i of block b forms
 * z_k = log(alpha / K_max + n_k) + log predictive_k(X[i]) over all K_max slots -- no lms on the prior term (fbgmm.py:475-479 has
 * none), the likelihood bits of segk_fbi_assign -- and takes k = the FIRST index of max_k z_k.  No temperature, no uniform, no
 * softmax, no `k > K` clamp (batch slots are slots); all empty slots of an item tie exactly and the first wins.  `sweep` is not
 * read (the caller still advances its counter, so that sampled sweeps after a MAP sweep use the uniforms they would have used).
 * bt->slot[i] and n_new[i] = 1 are written as by segk_fbi_assign.  *n_moved [dev] += the considered items whose slot after the
 * call differs from before (an unassigned item that gets a slot counts): one integer add per workgroup, so the sum does not
 * depend on launch order, and it accumulates over the launches of a block and over the blocks of a sweep; the caller zeroes it.
 * The prior terms are staged once per workgroup as a 65th row of the tile's logits: 65 K_max doubles in LDS next to the staged
 * rows where they fit in 144 KiB, else in the bounded workspace (SEGK_FBI_Z_MIB); cov_type 2 reads the token-likelihood table
 * and keeps the K_max prior terms alone in LDS.  Arguments, probe_ll and refusals otherwise as segk_fbi_assign: a language model
 * and the cov_type 2 limits SEGK_ERR_UNSUPPORTED, a corpus with span tables or D > 256 SEGK_ERR_ARG, all before any launch.      */
int32_t segk_fbi_assign_map(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt,
                            int32_t s_lo, int32_t s_n, int32_t b, const int32_t *n_items, uint64_t sweep,
                            int32_t consider_unassigned, const int32_t *new_tok, int32_t *n_new, double *probe_ll,
                            int64_t probe_ld, int32_t *n_moved, void *stream);
/* segk_fbi_assign_map on the float32 item likelihoods of segk_fbi_assign_diag32 (added at ABI 15 without a bump; the MAP sweeps
 * of FBGMM(..., score_precision="f32"); it replaces fbgmm.py:465-494 as segk_fbi_assign_map does): the likelihood half of
 * segk_fbi_assign_diag32, then the fp64 first argmax of log(alpha / K_max + n_k) + ll_k and the count of moved items exactly as
 * above; the tile's logits are 65 rows of K_max | 1 doubles.  Refused before any launch: cov_type 0 or 2 and a language model
 * with SEGK_ERR_UNSUPPORTED; bt->tab32, bt->centre or bt->prior_rows NULL, D > 256 or a corpus with span tables SEGK_ERR_ARG.   */
int32_t segk_fbi_assign_map_diag32(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt,
                                   int32_t s_lo, int32_t s_n, int32_t b, const int32_t *n_items, uint64_t sweep,
                                   int32_t consider_unassigned, const int32_t *new_tok, int32_t *n_new, double *probe_ll,
                                   int64_t probe_ld, int32_t *n_moved, void *stream);
/* Held-out rows against the fitted bank of the stand-alone mixture model (added at ABI 15 without a bump; FBGMM.predict,
 * score_samples, predict_log_proba; specification tests/fbgmm_predict.py).  The M rows of Xq [dev] (the dtype of c->X, ldq
 * elements between rows) are in no model; each is treated as an UNASSIGNED item appended to X, against the statistics of all
 * items that hold a slot -- `bt` in the state segk_fbb_prepare(-1) leaves (counts n_k, N_a = sum n_k in scal[0], the predictive
 * parameters of every slot).  With ll_k(x) the log predictive of slot k (an empty slot: the prior predictive of the row, which
 * the call evaluates into prior_rows_q [dev] [M] first -- cov_type 0 / 1 the arithmetic of segk_fbb_prior_rows, cov_type 2 that
 * of `cached_log_prior`, gaussian_components.py:125-127), per row:
 *   label [dev] [M]          the first index of max_k log(alpha / K_max + n_k) + ll_k -- map_assign_i's choice, fbgmm.py:475-488:
 *                            no lms, no softmax, all empty slots tie and the first wins -- in the numbering of the reference's
 *                            view: an occupied slot its rank among the occupied slots in increasing slot order (what
 *                            segk_fbb_canonical assigns), an empty slot K, "would found a new component" (:489-490);
 *   log_density [dev] [M]    logsumexp_k lms (log(alpha / K_max + n_k) - log(N_a + alpha)) + ll_k: log_marg_i of the appended
 *                            item, fbgmm.py:256-285;
 *   log_resp [dev]           log_resp[r * resp_ld + k] = lms log(alpha / K_max + n_k) + ll_k - logsumexp(.), the normalised
 *                            log_prob_z of fbgmm.py:436-451 at temperature 1, in SLOT order (the caller permutes columns).
 * Each of the three may be NULL.  probe_ll [dev] (tests; may be NULL): probe_ll[r * probe_ld + k] = ll_k of row r.  The call
 * reads the model and writes only its outputs and workspaces of the context: bt->slot, the partial sums, f->* and prior_c stay
 * as they are, no uniform and no sweep counter is read.  The likelihood bits are those segk_fbi_assign forms for the same row
 * and statistics (cov_type 2: segk_fcb_token_ll's, on a view of the query walked in chunks whose table stays within
 * SEGK_FBI_Z_MIB).  One launch per 64 rows x all slots; a tile's logits in LDS where rows, staged slots, the prior terms, the
 * rank table and logits fit in 144 KiB, else in the bounded workspace of segk_fbi_assign and several launches.
 * Refused before any launch: a language model, cov_type 2 beyond D <= 64 / K_max <= 1024 with SEGK_ERR_UNSUPPORTED; a corpus with
 * span tables, D > 256, NULL Xq or prior_rows_q with M > 0, resp_ld or probe_ld < K_max, missing slot tables with SEGK_ERR_ARG.
 * M = 0 returns SEGK_OK and launches nothing.                                                                              */
int32_t segk_fbi_predict(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, const void *Xq,
                         int64_t ldq, int64_t M, double *prior_rows_q, int32_t *label, double *log_density,
                         double *log_resp, int64_t resp_ld, double *probe_ll, int64_t probe_ld, void *stream);
/* segk_fbi_predict on the float32 item likelihoods of segk_fbi_assign_diag32 (added at ABI 15 without a bump; the model's
 * score_precision="f32"): fbb_term32 on float32 rows and bt->tab32, the centre subtracted in fp64, then the same fp64 epilogue
 * on logit rows of K_max | 1 doubles.  Refused before any launch: cov_type 0 or 2 and a language model with
 * SEGK_ERR_UNSUPPORTED; bt->tab32 or bt->centre NULL and the argument errors of segk_fbi_predict with SEGK_ERR_ARG.          */
int32_t segk_fbi_predict_diag32(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt,
                                const void *Xq, int64_t ldq, int64_t M, double *prior_rows_q, int32_t *label,
                                double *log_density, double *log_resp, int64_t resp_ld, double *probe_ll, int64_t probe_ld,
                                void *stream);
/* Held-out UTTERANCES against the fitted bank of the unigram segmenter (added at ABI 15 without a bump;
 * UnigramAcousticWordseg.decode; specification tests/wordseg_decode.py): the MAP boundaries and the transcript of every
 * utterance of `cq`, a corpus that is in no model -- its rows are the M candidate embeddings of the held-out utterances, its
 * span tables (triangles, and the complete band of segk_corpus.band_ids for n_slices_max where N_max > 64) index them.  The
 * caller has scored and labelled the rows with segk_fbi_predict / _predict_diag32 on `bt` in the state segk_fbb_prepare(-1)
 * leaves: density [dev] [M] = log_marg_i of the row appended as an unassigned item (fbgmm.py:256-285, lms included), label
 * [dev] [M] = map_assign_i's choice (fbgmm.py:475-490) in the reference view's numbering.  Per utterance i of N landmarks:
 *   vec[j] = density[id_j] * dur_j ** time_power_term + wip, -inf where id_j == -1 or dur_j is NaN
 *            (get_vec_embed_log_probs, unigram_acoustic_wordseg.py:474-511);
 *   boundaries [dev] uint8 [n_utt, N_max], log_prob [dev] [n_utt]: forward_backward_viterbi(vec, 0.0, N, n_slices_min,
 *            n_slices_max) (:759-864) from cleared flags -- among equal maxima the shortest span, the reference's stepping back
 *            from a dead end (:815-825); the flags beyond N are written 0;
 *   seg_embed / seg_label [dev] int32, seg_density [dev] double, each [n_utt, N_max]: per chosen segment, in landmark order,
 *            its embedding row id, label[id] and density[id]; a chosen segment whose span has no embedding (only after
 *            stepping back from a dead end) is kept as (-1, -1, -inf) so that segment j ends at the j-th set flag; the entries
 *            beyond the count are written (-1, -1, -inf);
 *   n_seg [dev] int32 [n_utt]: the number of chosen segments.
 * Every segment is labelled independently against the same statistics: nothing is added to the bank between segments (a
 * serial Viterbi visit, :252-360, would add each).  The call reads `cq`, density and label and writes its seven outputs:
 * no mixture model, no batch state, no old boundaries, no uniform, no temperature.  One launch, one workgroup per utterance,
 * no atomics; the kernel is a copy of the boundary kernel of segk_fbb_segment_map with the slot clearing and the token lists
 * taken out, in a unit of its own.  The layout is chosen from cq->N_max, whatever corpus the model was trained on.
 * SEGK_ERR_ARG before any launch: n_slices_min outside {0, 1}; N_max > 64 with n_slices_max == 0 or > 64, without a complete
 * band (band_ids / band_dur NULL or band_W != n_slices_max), or with a band beyond 160 KiB of LDS (12 N_max W + 24 N_max + 16 +
 * N_max rounded up to 16 bytes); N_max <= 64 without triangular tables; a NULL output.  n_utt == 0 returns SEGK_OK and
 * launches nothing.                                                                                                         */
int32_t segk_fbd_decode(segk_ctx *ctx, const segk_corpus *cq, int32_t n_slices_min, int32_t n_slices_max, double wip,
                        double time_power_term, const double *density, const int32_t *label, uint8_t *boundaries,
                        int32_t *seg_embed, int32_t *seg_label, double *seg_density, int32_t *n_seg, double *log_prob,
                        void *stream);
/* Held-out UTTERANCES against a fitted segmental k-means (added at ABI 15 without a bump; SegmentalKMeansWordseg.decode;
 * specification tests/kmeans_decode.py): segment_i (kmeans_acoustic_wordseg.py:225-332) of every utterance of `cq` up to and
 * without its update (:314-320) -- the reference scores an utterance's spans against the current means without removing its
 * own items and takes boundaries and labels (:288, :313) before it updates, so nothing differs from it.  `cq` is a corpus that
 * is in no model: its rows are the M candidate embeddings of the held-out utterances, its span tables index them.  The caller
 * has scored the rows with segk_kmeans_score(cq, m) into `cand`, a segk_cand of n_emb = M entries of its own: cand->k[row] =
 * argmax_neg_sqrd_norm_i (first maximum), cand->s[row] = max_neg_sqrd_norm_i over all K_max rows of m->means, inactive rows
 * included (kmeans_components.py:225-232).  Per utterance i of N landmarks:
 *   vec[j] = cand->s[id_j] * dur_j + wip, -inf where id_j == -1 or dur_j is NaN (get_vec_embed_neg_len_sqrd_norms, :334-351);
 *   boundaries [dev] uint8 [n_utt, N_max], objective [dev] double [n_utt]: forward_backward_kmeans_viterbi(vec, N,
 *            n_slices_min, n_slices_max) (:449-555) from cleared flags -- among equal maxima the shortest span, the reference's
 *            stepping back from a dead end (:521-533); the objective is summed in the backward walk's order; the flags beyond N
 *            are written 0;
 *   seg_embed / seg_row / seg_label [dev] int32, seg_score [dev] double, each [n_utt, N_max]: per chosen segment, in landmark
 *            order, its embedding row id, cand->k[id], min(cand->k[id], *m->K) -- the component add_item would give it
 *            (kmeans_components.py:103-106), K for "would found a new component" -- and cand->s[id], the unscaled
 *            max_neg_sqrd_norm; a chosen segment whose span has no embedding (only after stepping back from a dead end) is
 *            kept as (-1, -1, -1, -inf) so that segment j ends at the j-th set flag; the entries beyond the count are written
 *            (-1, -1, -1, -inf);
 *   n_seg [dev] int32 [n_utt]: the number of chosen segments.
 * The call reads cq, cand->k, cand->s and m->K and writes its seven outputs: no old boundaries, no token lists, no flag counts,
 * no status word, nothing of the model.  One launch, one wave per utterance, no atomics: for N_max <= 64 and windows 1..8 the
 * register DP of segk_kmeans_segment's fast path, otherwise its generic walk (any N_max, n_slices_max == 0, windows above 8).
 * The layout is chosen from cq->N_max, whatever corpus the model was trained on.
 * SEGK_ERR_ARG before any launch: n_slices_min outside {0, 1}; n_slices_max < 0; a corpus without span tables; a NULL
 * argument.  SEGK_ERR_UNSUPPORTED before any launch: a band of N_max x W spans (W = n_slices_max, or N_max without a window)
 * beyond the 160 KiB of LDS of a workgroup (generic: 12 N_max W + 9 N_max + 8 bytes rounded up to 16).  n_utt == 0 returns
 * SEGK_OK and launches nothing.                                                                                             */
int32_t segk_kmd_decode(segk_ctx *ctx, const segk_corpus *cq, const segk_kmeans *m, const segk_cand *cand, int32_t n_slices_min,
                        int32_t n_slices_max, double wip, uint8_t *boundaries, int32_t *seg_embed, int32_t *seg_row,
                        int32_t *seg_label, double *seg_score, int32_t *n_seg, double *objective, void *stream);
/* Acoustic-model batch sweeps of the unigram segmenter (added at ABI 15 without a bump; the inner sweeps of
 * UnigramAcousticWordseg.gibbs_sample(n, am_n_iter=m), unigram_acoustic_wordseg.py:440-443 -- FBGMM.gibbs_sample(m,
 * consider_unassigned=False) over the currently assigned tokens -- as a blocked sampler on the segmenter's batch state;
 * specification tests/am_batch.py).  A sweep is the sweep of segk_fbb_* above with the span scores and the boundary step left
 * out: per block b segk_fbb_prepare(b), this call, segk_fbb_partials(b).  This call is step b's token half on a corpus WITH
 * utterances (span tables present, any N_max, band corpora included): every current token (i, t) of the utterances of block b
 * of the local slices [s_lo, s_lo + s_n) -- row new_tok[i * N_max + t], t < n_new[i] -- forms
 * z_k = lms log(alpha / K_max + n_k) + log predictive_k(row) over all K_max slots (an empty slot: bt->prior_rows[row]), anneals
 * it when anneal_temp != 1 (fbgmm.py:446-449) and draws its slot by the inverse-CDF walk on u01(bt->seed, sweep, i, N_max + t):
 * the uniforms, likelihood bits and draws of segk_fbb_assign on the same token lists and statistics.  Only bt->slot[row] is
 * written: new_tok, n_new, the boundaries and out_logprob are not.
 * A first kernel (one workgroup per local slice, an ordered scan of n_new, no atomics) compacts the cell's tokens, in utterance
 * order, into a workspace of the context; the tile kernel of segk_fbi_assign then takes 64 tokens per workgroup against all
 * slots.  Nothing is read back: tok_cap [host] [s_n], the landmarks of the cell's utterances (an upper bound on its tokens, at
 * most n_utts[s] * N_max), sizes the grid, and a tile beyond the device-side count returns at once.  n_utts [host] [s_n]: the
 * utterances of block b per local slice.  cov_type 0, 1 (D <= 256) and 2 (D <= 64, K_max <= 1024; the likelihoods by the
 * token-likelihood kernel of segk_fbb_assign); X float32 or float64; fp64 arithmetic; the logits in LDS or the bounded workspace
 * of segk_fbi_assign (SEGK_FBI_Z_MIB).  A language model (f->lm_unigram) and the cov_type 2 limits are SEGK_ERR_UNSUPPORTED, a
 * corpus without span tables or D > 256 SEGK_ERR_ARG, all before any launch.  probe_ll (NULL in production) receives the
 * likelihood part of the logits in the layout of segk_fbb_set_probe's ll_out: probe_ll[(i * N_max + t) * probe_ld + k].        */
int32_t segk_fbt_assign(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt,
                        int32_t s_lo, int32_t s_n, int32_t b, const int32_t *n_utts, const int32_t *tok_cap,
                        uint64_t sweep, double anneal_temp, const int32_t *new_tok, const int32_t *n_new,
                        double *probe_ll, int64_t probe_ld, void *stream);
/* segk_fbt_assign for diagonal components (cov_type 1) with float32 token likelihoods (added at ABI 15 without a bump; the
 * inner sweeps of UnigramAcousticWordseg.gibbs_sample(..., am_sync="batch", am_score_precision="f32"); specification
 * tests/am_batch.py, emulation tests/am_batch_f32.py).  It replaces what segk_fbt_assign replaces -- fbgmm.py:422-463 over the
 * tokens, the inner sweeps of unigram_acoustic_wordseg.py:440-443 -- with the same arguments, the same role in a step (after
 * segk_fbb_prepare(b), which writes bt->tab32, before segk_fbb_partials(b)) and the same writes: bt->slot[row] of every
 * current token and nothing else.  Only the likelihood half differs, exactly as segk_fbi_assign_diag32 differs from
 * segk_fbi_assign: m = float(mean - centre), q = float(q) from bt->tab32, x = float(X[row][d] - centre[d]) with the difference
 * in fp64, acc += log2(1 + (m - x)^2 q) on the hardware logarithm, dimensions ascending, ll = lconst - half * (ln 2 * acc) in
 * fp64; an empty slot keeps bt->prior_rows[row].  Logits, prior term, softmax, annealing and the inverse-CDF walk on
 * u01(bt->seed, sweep, i, N_max + t) are fp64: the draws are the fp64 function of likelihoods within the tolerance contract
 * (1e-4 max(|ll|, 1)) of segk_fbt_assign's; segk_fbb_assign_diag32 on the same token lists forms the same term in the same
 * order of dimensions (both are held to the contract, not to each other's bits).  The token lists are segk_fbt_assign's (the same compaction kernel and workspace);
 * the tile kernel is segk_fbi_assign_diag32's with the rows gathered through them; LDS and the bounded workspace
 * (SEGK_FBI_Z_MIB) as there.  Refused before any launch: cov_type 0 or 2 and a language model with SEGK_ERR_UNSUPPORTED;
 * bt->tab32, bt->centre or bt->prior_rows NULL, a corpus without span tables or D > 256 with SEGK_ERR_ARG.  probe_ll as for
 * segk_fbt_assign.                                                                                                            */
int32_t segk_fbt_assign_diag32(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt,
                               int32_t s_lo, int32_t s_n, int32_t b, const int32_t *n_utts, const int32_t *tok_cap,
                               uint64_t sweep, double anneal_temp, const int32_t *new_tok, const int32_t *n_new,
                               double *probe_ll, int64_t probe_ld, void *stream);
/* The orphan pass of FBGMM.set_K(K, sync="batch") (added at ABI 15 without a bump; it replaces fbgmm.py:174-180, the loop that
 * re-homes, one gibbs_sample_inside_loop_i after the other, every item whose component went when the bank was cut to its K
 * largest; specification tests/fbgmm_set_k.py).  The arguments and the corpus of items are segk_fbi_assign's.  This call is the
 * item half of step b of the pass, after segk_fbb_prepare(-1) -- the statistics of every item that holds a slot, in all blocks: an
 * orphan holds none, so nothing is left out -- and before segk_fbb_partials(b): every ORPHAN i of block b of the local slices
 * [s_lo, s_lo + s_n) -- was[i] >= 0 and bt->slot[i] < 0 -- forms segk_fbi_assign's logits at temperature 1 and draws its slot on
 * u01(bt->seed, sweep, i, 1): the likelihood bits and the draw segk_fbi_assign would give item i on the same statistics.
 * bt->slot[i] and n_new[i] = 1 are written; every other item is left alone (an item with was[i] < 0 keeps -1).
 * was [dev] int32 [n_emb]: the assignments before the cut (any value >= 0: the item was assigned).
 * A first kernel (one workgroup per local slice, an ordered scan, no atomics) compacts the ids of the cell's orphans, in index
 * order, into the workspace of segk_fbt_assign and marks their n_new; the tile kernel of segk_fbi_assign then takes 64 listed
 * items per workgroup against all slots, the rows gathered through the list.  Nothing is read back: n_items [host] [s_n] (the
 * cell's items, an upper bound on its orphans) sizes the grid, and a tile beyond the device-side count returns at once.  With
 * cov_type 2 the token-likelihood kernel of segk_fbb_assign runs over the block's items that n_new names (the orphans and the
 * items that kept their slot), the tile kernel draws for the listed ones.  The likelihoods are fp64 whatever bt->tab32 holds.
 * The logits in LDS or the bounded workspace of segk_fbi_assign (SEGK_FBI_Z_MIB).  A language model (f->lm_unigram) and the
 * cov_type 2 limits are SEGK_ERR_UNSUPPORTED, a corpus with span tables or D > 256 SEGK_ERR_ARG, all before any launch.
 * probe_ll as for segk_fbi_assign, the rows of the listed items only.                                                          */
int32_t segk_fbi_assign_orphans(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt,
                                int32_t s_lo, int32_t s_n, int32_t b, const int32_t *n_items, uint64_t sweep,
                                const int32_t *was, const int32_t *new_tok, int32_t *n_new, double *probe_ll,
                                int64_t probe_ld, void *stream);
/* bigram table += sign * (transcripts of block b, all slices) from bt->lm_tok                  */
int32_t segk_fbb_lm_apply(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f,
                          const segk_fbatch *bt, int32_t b, int32_t sign, void *stream);
/* bt->lm_tok[b][s] <- slots of the new tokens of the local slices                              */
int32_t segk_fbb_lm_fill(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f,
                         const segk_fbatch *bt, int32_t s_lo, int32_t s_n, int32_t b,
                         const int32_t *n_utts, const int32_t *new_tok, const int32_t *n_new,
                         void *stream);
/* after segk_fbb_prepare(b = -1): remap [dev] [K_max] occupied slots -> 0..K-1 in increasing slot
 * order (-1 for empty), f->assignments[row] = remap[slot[row]], *f->K = K.                      */
int32_t segk_fbb_canonical(segk_ctx *ctx, const segk_corpus *c, segk_fbgmm *f,
                           const segk_fbatch *bt, int32_t *remap, void *stream);

/* -------------------------------------------------------------------------------------
 * A6 / A7 / A8 on caller-supplied score vectors -- drop-in for the module-level functions
 *   kind 0: forward_backward_kmeans_viterbi   kmeans_acoustic_wordseg.py:449-555
 *   kind 1: forward_backward_viterbi          unigram_acoustic_wordseg.py:759-864
 *   kind 2: forward_backward                  unigram_acoustic_wordseg.py:653-756
 * n_prob independent problems; problem p has Ns[p] landmarks and its triangular vector
 * (N(N+1)/2 doubles, entry t(t-1)/2+s = span [s,t)) starts at vecs + offs[p].  kind 2
 * consumes uniforms[p*u_stride + j] in place of the j-th random.random() call
 * (_cython_utils.pyx:83) and reports the number consumed in n_draws[p]; status[p] = 1 where
 * the reference would `assert False` (log_prob == -inf, :753).
 *   bounds [dev] uint8 [n_prob, b_stride], totals [dev] double [n_prob],
 *   work [dev] double [n_prob, w_stride], w_stride >= 3*N_max + 2.
 * ------------------------------------------------------------------------------------- */
int32_t segk_dp_tri(segk_ctx *ctx, int32_t kind, const double *vecs, const int32_t *Ns,
                    const int64_t *offs, int32_t n_prob, int32_t n_slices_min, int32_t n_slices_max,
                    double log_p_continue, double anneal_temp, const double *uniforms,
                    int64_t u_stride, uint8_t *bounds, int64_t b_stride, double *totals,
                    int32_t *n_draws, int32_t *status, double *work, int64_t w_stride, void *stream);

/* -------------------------------------------------------------------------------------
 * A9 host shims -- _cython_utils.pyx:13-25 (logsumexp), :75-89 (draw, uniform supplied by
 * the caller instead of random.random()), :30-70 (sums).  Pure host functions on [host]
 * buffers, kept so that `segmentalist_amd._cython_utils` is a drop-in module.
 * ------------------------------------------------------------------------------------- */
double segk_logsumexp(const double *a, int64_t n);
int32_t segk_draw(const double *p_k, int64_t n, double u);
double segk_sum_doubles(const double *y, int64_t n);
int64_t segk_sum_ints(const int64_t *y, int64_t n);
double segk_sum_log(const double *y, int64_t n);
double segk_sum_square_a_times_b(const double *a, const double *b, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* SEGK_H */
