// segk_fbdecode.hip -- the boundary step of UnigramAcousticWordseg.decode (segk_fbd_decode; specification
// tests/wordseg_decode.py): MAP boundaries and the transcript of HELD-OUT utterances, read-only.
//
// A held-out utterance is in no model: its candidate embeddings are rows of a query matrix, scored and labelled against the
// frozen statistics by segk_fbi_predict / _predict_diag32 (density[row] = log_marg_i of the row appended as an unassigned item,
// label[row] = map_assign_i's choice in the reference view's numbering).  This unit turns those two arrays into boundaries:
//
//   k_fbd_decode<BAND>   one utterance of the held-out corpus per workgroup of 128 threads; wave 0 runs the DP.  A read-only
//                        sibling of k_fbb_segment<BAND, true> (segk_fbbatch.hip), kept as a copy in a unit of its own so that
//                        the generated code of every other unit stays what it was: the span ids and
//                        vec[j] = density[id] * dur ** time_power_term + wip (unigram_acoustic_wordseg.py:474-511) are staged in
//                        LDS -- triangles where the held-out corpus has N_max <= 64, its band [N][W] beyond (fb_fill_vec /
//                        fb_fill_vec_band) --, the max-plus DP with backpointers (fb_dp_viterbi_on, :759-864) starts from
//                        cleared flags, and from the final flags the wave writes the boundary row, per chosen segment in
//                        landmark order (embedding row, label[row], density[row]) -- a segment whose span has no embedding,
//                        which back-tracking from a dead end can leave, is kept as (-1, -1, -inf) so that segments and
//                        boundaries stay aligned --, the segment count and the DP total.
//
// It reads no batch state and no mixture model, clears no slots, reads no old boundaries.  No atomics, no grid barrier, no
// spin loop, vector stores only: a plain grid over the utterances.
// LDS, `cells` = N_max W (band) or N_max (N_max + 1) / 2 (triangle) -- fbd_lds is its size on the host, k_fbb_segment's
// without the old token list:
//   vec [cells], a [N_max], bp [N_max + 1], spare [N_max + 1] (double rows; bp holds int32); ids [cells] (int32); bnd [N_max]
//   (bytes, rounded up to 16)
#include "segk_fb_common.h"

#define FBD_BAND_LDS_MAX (160 * 1024)

static size_t fbd_lds(int64_t NM, int64_t W, bool band)
{
    const int64_t cells = band ? NM * W : NM * (NM + 1) / 2;
    return (size_t)(cells + 3 * NM + 2) * sizeof(double) + (size_t)cells * sizeof(int32_t) + (size_t)((NM + 15) & ~15);
}

template <bool BAND>
__global__ __launch_bounds__(128) void k_fbd_decode(segk_corpus c, int n_max, double wip, double time_power_term, const double *density,
                                                    const int32_t *label, uint8_t *boundaries, int32_t *seg_embed, int32_t *seg_label,
                                                    double *seg_density, int32_t *n_seg, double *log_prob)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int utt = blockIdx.x;
    if (utt >= c.n_utt) return;
    const int NM = c.N_max;
    int N = c.lengths[utt];
    N = N < 0 ? 0 : (N > NM ? NM : N);                 // (the tables of an utterance hold N_max landmarks)
    [[maybe_unused]] const int W = c.band_W;           // the band's columns (BAND only)
    const int tri = N * (N + 1) / 2;
    const int64_t cells = BAND ? (int64_t)NM * W : (int64_t)NM * (NM + 1) / 2;
    double *vec = (double *)smem;                      // [cells]
    double *a = vec + cells;                           // [N_max]
    double *w = a + NM;                                // [N_max + 1]: the backpointers
    int32_t *ids = (int32_t *)(w + 2 * (NM + 1));      // [cells]
    uint8_t *bnd = (uint8_t *)(ids + cells);           // [N_max]
    const int64_t row = (int64_t)utt * NM;
    if (N == 0) {                                      // an utterance without landmarks: no segment, an empty sum
        for (int j = threadIdx.x; j < NM; j += blockDim.x) {
            boundaries[row + j] = 0;
            seg_embed[row + j] = -1;
            seg_label[row + j] = -1;
            seg_density[row + j] = NEG_INF_D;
        }
        if (threadIdx.x == 0) {
            n_seg[utt] = 0;
            log_prob[utt] = 0.0;
        }
        return;
    }
    const auto score_of = [&](int id) { return density[id]; };
    if constexpr (BAND) {
        fb_fill_vec_band(c.band_ids + row * W, c.band_dur + row * W, N, W, score_of, time_power_term, wip, vec, ids, threadIdx.x,
                         blockDim.x);
    } else {
        const FbSpanTab tab = fb_span_tab(c, utt, N, n_max);
        if (tab.band) {
            for (int j = threadIdx.x; j < tri; j += blockDim.x) ids[j] = -1;
            __syncthreads();
            const int Wt = tab.W;
            for (int i = threadIdx.x; i < N * Wt; i += blockDim.x) {
                const int t = i / Wt + 1, s2 = t - 1 - (i - (t - 1) * Wt);
                if (s2 >= 0) ids[t * (t - 1) / 2 + s2] = tab.bandi[i];
            }
        } else {
            for (int j = threadIdx.x; j < tri; j += blockDim.x) ids[j] = tab.vid[j];
        }
        fb_fill_vec(tab, N, tri, score_of, time_power_term, wip, vec, threadIdx.x, blockDim.x);
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    double total;
    if constexpr (BAND) total = fb_dp_viterbi_on(FbBandVec{vec, W, N}, a, (int32_t *)w, N, W, bnd, lane);
    else total = fb_dp_viterbi_on(FbTriVec{vec, tri}, a, (int32_t *)w, N, n_max, bnd, lane);
    // (the boundary flags were written by lane 0 of this wave)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // the chosen segments, 64 flags at a time: the lane of every set flag looks up its own segment [jp, j + 1); the position
    // behind the last set flag and the running segment count are carried from chunk to chunk (fb_collect_tokens_wave_band, with
    // the segments that have no embedding kept)
    int ns = 0, start = 0;
    for (int c0 = 0; c0 < N; c0 += 64) {
        const int j = c0 + lane;
        const uint8_t flag = j < N ? __hip_atomic_load(&bnd[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : (uint8_t)0;
        const unsigned long long mask = __ballot(flag != 0);
        const bool bit = j < N && ((mask >> lane) & 1ull);
        const unsigned long long below = mask & ((1ull << lane) - 1ull);
        const int jp = below ? c0 + 64 - __clzll((long long)below) : start;
        if (bit) {
            int id = -1;
            if constexpr (BAND) {
                if (j - jp < W) id = ids[(int64_t)j * W + (j - jp)];
            } else {
                id = ids[(j + 1) * j / 2 + jp];
            }
            const int64_t o = row + ns + __popcll(below);
            seg_embed[o] = id;
            seg_label[o] = id >= 0 ? label[id] : -1;
            seg_density[o] = id >= 0 ? density[id] : NEG_INF_D;
        }
        ns += __popcll(mask);
        if (mask) start = c0 + 64 - __clzll((long long)mask);
    }
    for (int j = ns + lane; j < NM; j += 64) {         // the rest of the row: no segment
        seg_embed[row + j] = -1;
        seg_label[row + j] = -1;
        seg_density[row + j] = NEG_INF_D;
    }
    for (int j = lane; j < NM; j += 64) boundaries[row + j] = j < N ? bnd[j] : (uint8_t)0;
    if (lane != 0) return;
    n_seg[utt] = ns;
    log_prob[utt] = total;
}

// What a held-out corpus with an utterance of more than 64 landmarks needs (N_max <= 64: nothing): check_fbb_long of
// segk_fbbatch.hip on this kernel's LDS
static int check_fbd_long(const segk_corpus *c, int n_slices_max)
{
    if (c->N_max <= 64) return SEGK_OK;
    if (n_slices_max <= 0 || n_slices_max > 64) {
        segk_set_error("segk_fbd_decode takes utterances of more than 64 landmarks (N_max = %d) with a window of 1..64 slices only "
                       "(n_slices_max = %d): set n_slices_max", c->N_max, n_slices_max);
        return SEGK_ERR_ARG;
    }
    if (!c->band_ids || !c->band_dur || c->band_W != n_slices_max) {
        segk_set_error("segk_fbd_decode takes utterances of more than 64 landmarks (N_max = %d) only when no span longer than the "
                       "window has an embedding (no complete band for n_slices_max = %d): build the corpus for this window",
                       c->N_max, n_slices_max);
        return SEGK_ERR_ARG;
    }
    const size_t lds = fbd_lds(c->N_max, c->band_W, true);
    if (lds > FBD_BAND_LDS_MAX) {
        segk_set_error("the banded span table of the longest utterance does not fit in LDS: N_max = %d landmarks, window W = %d: "
                       "12 N_max W + 24 N_max + 16 + (N_max rounded up to 16) = %zu bytes needed, %d available: shorten the "
                       "window (n_slices_max) or split the longest utterances", c->N_max, c->band_W, lds, FBD_BAND_LDS_MAX);
        return SEGK_ERR_ARG;
    }
    return SEGK_OK;
}

extern "C" {

int32_t segk_fbd_decode(segk_ctx *ctx, const segk_corpus *cq, int32_t n_slices_min, int32_t n_slices_max, double wip,
                        double time_power_term, const double *density, const int32_t *label, uint8_t *boundaries,
                        int32_t *seg_embed, int32_t *seg_label, double *seg_density, int32_t *n_seg, double *log_prob, void *stream)
{
    SEGK_REQUIRE(ctx && cq, "NULL context / held-out corpus");
    SEGK_REQUIRE(n_slices_min == 0 || n_slices_min == 1, "n_slices_min must be 0 or 1");
    SEGK_REQUIRE(n_slices_max >= 0, "n_slices_max must be >= 0 (0: no window)");
    SEGK_REQUIRE(cq->n_utt >= 0, "n_utt");
    if (cq->n_utt == 0) return SEGK_OK;
    SEGK_REQUIRE(cq->N_max > 0 && cq->lengths, "held-out corpus without landmarks");
    if (int rc = check_fbd_long(cq, n_slices_max)) return rc;
    const bool band = cq->N_max > 64;
    SEGK_REQUIRE(band || (cq->vec_ids && cq->durations), "held-out corpus without span tables");
    SEGK_REQUIRE(density && label && boundaries && seg_embed && seg_label && seg_density && n_seg && log_prob, "NULL argument");
    const size_t lds = fbd_lds(cq->N_max, cq->band_W, band);
    if (band) {
        SEGK_CHECK_HIP(segk_dyn_lds((const void *)k_fbd_decode<true>, lds));
        hipLaunchKernelGGL((k_fbd_decode<true>), dim3((unsigned)cq->n_utt), dim3(128), lds, (hipStream_t)stream, *cq, n_slices_max, wip,
                           time_power_term, density, label, boundaries, seg_embed, seg_label, seg_density, n_seg, log_prob);
    } else {
        SEGK_CHECK_HIP(segk_dyn_lds((const void *)k_fbd_decode<false>, lds));
        hipLaunchKernelGGL((k_fbd_decode<false>), dim3((unsigned)cq->n_utt), dim3(128), lds, (hipStream_t)stream, *cq, n_slices_max, wip,
                           time_power_term, density, label, boundaries, seg_embed, seg_label, seg_density, n_seg, log_prob);
    }
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

}  // extern "C"
