// segk_kmdecode.hip -- the boundary step of SegmentalKMeansWordseg.decode (segk_kmd_decode; specification
// tests/kmeans_decode.py): boundaries, objective and transcript of HELD-OUT utterances, read-only.
//
// A held-out utterance is in no model: its candidate embeddings are the rows of a corpus of their own, scored against the
// model's means by segk_kmeans_score into a segk_cand of the call's own (cand.k[row] = argmax_neg_sqrd_norm_i, cand.s[row] =
// max_neg_sqrd_norm_i over all K_max rows of `means`, kmeans_components.py:225-232).  This unit turns those two arrays into
// boundaries -- segment_i (kmeans_acoustic_wordseg.py:225-332) up to and without its update (:314-320):
//
//   k_kmd_decode<FAST>   one utterance of the held-out corpus per WAVE.  A read-only sibling of k_kmeans_segment_w8 (FAST) and
//                        k_kmeans_segment (generic; segk_segment.hip), kept as a copy in a unit of its own so that the
//                        generated code of every other unit stays what it was.  The lanes gather the band of span ids and
//                        vec[j] = cand.s[id] * dur + wip (:334-351); the max-plus DP with the reference's stepping back from
//                        a dead end (:449-555) starts from cleared flags -- FAST (N_max <= 64, windows 1..8): the register DP
//                        seg_w8_uniform of segk_segment_dev.h; generic (any N_max, no window, windows above 8): lane 0 walks
//                        the band in LDS --; the objective is summed in the backward walk's order.  From the final flags the
//                        wave writes the boundary row and per chosen segment, in landmark order, (embedding row, cand.k[row],
//                        min(cand.k[row], K), cand.s[row]).  A chosen segment is looked up in the band, or in the triangular
//                        table when it is longer than the window (only after stepping back from a dead end); one whose span
//                        has no embedding is kept as (-1, -1, -1, -inf) so that segments and boundaries stay aligned.
//
// It reads no old boundaries, writes no token lists, no flag counts and no status word.  No atomics, no grid barrier, no spin
// loop, vector stores only: a plain grid over the utterances.
// LDS per wave, Wc = n_slices_max when 0 < n_slices_max < N_max, else N_max; cells = N_max Wc -- kmd_lds is its size on the host:
//   FAST      bvec [N_max][8], gam [N_max + 12] (double); bk [cells], bid [cells], l_new [N_max], l_newk [N_max], l_cnt [8] (int32)
//   generic   bvec [cells], gam [N_max + 1] (double); bid [cells] (int32); bnd [N_max] (bytes)
// each rounded up to 16 bytes.
#include "segk_kmeans_dev.h"
#include "segk_segment_dev.h"

#define KMD_LDS_MAX (160 * 1024)

static size_t kmd_lds(int64_t NM, int64_t Wc, bool fast)
{
    const int64_t cells = NM * Wc;
    const size_t b = fast ? (size_t)(9 * NM + 12) * sizeof(double) + (size_t)(2 * cells + 2 * NM + 8) * sizeof(int32_t)
                          : (size_t)(cells + NM + 1) * sizeof(double) + (size_t)cells * sizeof(int32_t) + (size_t)NM;
    return (b + 15) & ~(size_t)15;
}

template <bool FAST>
__global__ __launch_bounds__(256) void k_kmd_decode(segk_corpus c, const int32_t *Kp, int n_max, double wip, segk_cand cand,
                                                    uint8_t *boundaries, int32_t *seg_embed, int32_t *seg_row, int32_t *seg_label,
                                                    double *seg_score, int32_t *n_seg, double *objective, int cells, int wave_bytes)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int u = blockIdx.x * (blockDim.x >> 6) + wv;
    if (u >= c.n_utt) return;
    const int NM = c.N_max;
    int N = c.lengths[u];
    N = N < 0 ? 0 : (N > NM ? NM : N);                 // (the tables of an utterance hold N_max landmarks)
    const int64_t row = (int64_t)u * NM;
    if (N == 0) {                                      // an utterance without landmarks: no segment, an empty sum
        for (int j = lane; j < NM; j += 64) {
            boundaries[row + j] = 0;
            seg_embed[row + j] = -1;
            seg_row[row + j] = -1;
            seg_label[row + j] = -1;
            seg_score[row + j] = NEG_INF_D;
        }
        if (lane == 0) {
            n_seg[u] = 0;
            objective[u] = 0.0;
        }
        return;
    }
    const int W = (n_max > 0 && n_max < N) ? n_max : N;          // FAST: <= 8 (the host checks n_max <= 8)
    const int64_t triMax = (int64_t)NM * (NM + 1) / 2;
    const int32_t *vid = c.vec_ids + (int64_t)u * triMax;
    const double *dur = c.durations + (int64_t)u * triMax;
    // banded span tables (segk_corpus.band_ids / band_dur), when they were built for this window
    const bool band = c.band_ids != nullptr && c.band_W == W && W > 0;
    const int32_t *bandi = band ? c.band_ids + row * c.band_W : nullptr;
    const double *bandd = band ? c.band_dur + row * c.band_W : nullptr;
    const int Kact = *Kp;
    char *base = smem + (size_t)wv * wave_bytes;

    if constexpr (FAST) {
        double *bvec = (double *)base;                    // [N_max][8]: the DP's candidates, pitch 8, -inf beyond the window
        double *gam = bvec + NM * 8;                      // [8 + N_max + 4]
        int32_t *bk = (int32_t *)(gam + NM + 12);         // [cells]
        int32_t *bid = bk + cells;                        // [cells]
        int32_t *l_new = bid + cells;                     // [N_max]
        int32_t *l_newk = l_new + NM;                     // [N_max]
        int32_t *l_cnt = l_newk + NM;                     // [8]
        // the band (kmeans_acoustic_wordseg.py:334-351): lane (r, w) takes entry (r + 1, w), 32 span ends per batch: every
        // span id first, then every gather (k_kmeans_segment_w8)
        {
            const int w = lane & 7;
            for (int z0 = 0; z0 < N; z0 += 32) {
                int id[4], kq[4];
                double dd[4], sc[4];
#pragma unroll
                for (int z = 0; z < 4; z++) {
                    const int r = z0 + 8 * z + (lane >> 3), t = r + 1, sp = t - 1 - w;
                    id[z] = -1;
                    dd[z] = 0.0;
                    if (r < N && w < W && sp >= 0) {
                        const int j = t * (t - 1) / 2 + sp;
                        id[z] = band ? bandi[r * W + w] : vid[j];
                        dd[z] = band ? bandd[r * W + w] : dur[j];
                    }
                }
#pragma unroll
                for (int z = 0; z < 4; z++) {
                    kq[z] = -1;
                    sc[z] = 0.0;
                    if (id[z] >= 0) {
                        kq[z] = cand.k[id[z]];
                        sc[z] = cand.s[id[z]];
                    }
                }
#pragma unroll
                for (int z = 0; z < 4; z++) {
                    const int r = z0 + 8 * z + (lane >> 3);
                    if (r < N) {
                        double v = NEG_INF_D;
                        if (id[z] >= 0) v = isnan(dd[z]) ? NEG_INF_D : sc[z] * dd[z];      // :346-349
                        if (w < W) {
                            bid[r * W + w] = id[z];
                            bk[r * W + w] = kq[z];
                        }
                        bvec[r * 8 + w] = v + wip;                                          // :351
                    }
                }
            }
        }
        WAVE_SYNC();
        double total;
        unsigned long long newb, keep_;
        int id, rk, x_, f_;
        seg_w8_uniform(bvec, gam, bid, bk, N, W, Kact, l_new, l_newk, l_cnt, &total, lane, newb, keep_, id, rk, x_, f_);
        // the chosen segments: the lane of set flag j holds its own segment [jp, j + 1) (seg_w8_uniform: row and component of a
        // span inside the window; -1 otherwise); a span longer than the window comes from the triangular table
        const bool bit = lane < N && ((newb >> lane) & 1ull);
        const unsigned long long below = newb & ((1ull << lane) - 1ull);
        const int jp = below ? 64 - __clzll((long long)below) : 0;
        if (bit) {
            if (id < 0) rk = -1;
            if (lane - jp >= W) {
                id = vid[(lane + 1) * lane / 2 + jp];
                rk = id >= 0 ? cand.k[id] : -1;
            }
            const int64_t o = row + __popcll(below);
            seg_embed[o] = id;
            seg_row[o] = rk;
            seg_label[o] = rk < 0 ? -1 : (rk < Kact ? rk : Kact);            // add_item's clamp (kmeans_components.py:103-106)
            seg_score[o] = id >= 0 ? cand.s[id] : NEG_INF_D;
        }
        const int ns = __popcll(newb);
        for (int j = ns + lane; j < NM; j += 64) {         // the rest of the row: no segment
            seg_embed[row + j] = -1;
            seg_row[row + j] = -1;
            seg_label[row + j] = -1;
            seg_score[row + j] = NEG_INF_D;
        }
        if (lane < NM) boundaries[row + lane] = lane < N ? (uint8_t)((newb >> lane) & 1ull) : (uint8_t)0;
        if (lane == 0) {
            n_seg[u] = ns;
            objective[u] = total;
        }
    } else {
        double *bvec = (double *)base;                    // [cells]: entry (t, w) at [(t - 1) * W + w]
        double *gam = bvec + cells;                       // [N_max + 1]
        int32_t *bid = (int32_t *)(gam + NM + 1);         // [cells]
        uint8_t *l_bnd = (uint8_t *)(bid + cells);        // [N_max]
        const int nb = N * W;
        for (int i = lane; i < nb; i += 64) {
            const int t = i / W + 1, w = i % W, s = t - 1 - w;
            int id = -1;
            double v = NEG_INF_D;
            if (s >= 0) {
                const int64_t j = (int64_t)t * (t - 1) / 2 + s;
                id = band ? bandi[i] : vid[j];               // banded image: lane i reads entry i
                if (id >= 0) {
                    const double dd = band ? bandd[i] : dur[j];
                    v = isnan(dd) ? NEG_INF_D : cand.s[id] * dd;      // :346-349
                }
            }
            bid[i] = id;
            bvec[i] = v + wip;                                       // :351
        }
        WAVE_SYNC();
        double total = 0.0;
        if (lane == 0) {
#define V_(t, s) bvec[((t) - 1) * W + ((t) - 1 - (s))]
            // ---- forward (kmeans_acoustic_wordseg.py:494-506)
            gam[0] = 0.0;
            for (int t = 1; t < N; t++) {
                const int lo = t - W < 0 ? 0 : t - W;
                double best = NEG_INF_D;
                for (int s = lo; s < t; s++) {
                    const double v = V_(t, s) + gam[s];
                    if (v > best) best = v;
                }
                gam[t] = best;
            }
            for (int j = 0; j < N; j++) l_bnd[j] = 0;
            l_bnd[N - 1] = 1;
            // ---- backward (:510-553)
            int t = N, lo = 0;
            for (;;) {
                lo = t - W < 0 ? 0 : t - W;
                bool all_inf = true;
                for (int s = lo; s < t; s++)
                    if (V_(t, s) + gam[s] != NEG_INF_D) { all_inf = false; break; }
                if (all_inf) {
                    while (all_inf) {
                        t = t - 1;
                        if (t == 0) break;
                        lo = t - W < 0 ? 0 : t - W;
                        all_inf = true;
                        for (int s = lo; s < t; s++)
                            if (V_(t, s) + gam[s] != NEG_INF_D) { all_inf = false; break; }
                    }
                    l_bnd[(t - 1 + N) % N] = 1;
                }
                int k = 1;
                if (t > 0) {
                    double best = NEG_INF_D;
                    bool first = true;
                    for (int s = t - 1; s >= lo; s--) {
                        const double v = V_(t, s) + gam[s];
                        if (first || v > best) { best = v; k = t - s; first = false; }
                    }
                    total += V_(t, t - k);
                } else {
                    total += V_(N, N - 1);      // python vec[-1]: the last span [N-1, N)
                }
                if (t - k - 1 < 0) break;
                l_bnd[t - k - 1] = 1;
                t = t - k;
            }
#undef V_
        }
        WAVE_SYNC();
        // the chosen segments, 64 flags at a time: the lane of every set flag looks up its own segment [jp, j + 1); the position
        // behind the last set flag and the running segment count are carried from chunk to chunk
        int ns = 0, start = 0;
        for (int c0 = 0; c0 < N; c0 += 64) {
            const int j = c0 + lane;
            const unsigned long long mask = __ballot(j < N && l_bnd[j < N ? j : 0] != 0);
            const bool bit = j < N && ((mask >> lane) & 1ull);
            const unsigned long long below = mask & ((1ull << lane) - 1ull);
            const int jp = below ? c0 + 64 - __clzll((long long)below) : start;
            if (bit) {
                const int w = j - jp;
                const int id = w < W ? bid[j * W + w] : vid[(int64_t)(j + 1) * j / 2 + jp];
                const int rk = id >= 0 ? cand.k[id] : -1;
                const int64_t o = row + ns + __popcll(below);
                seg_embed[o] = id;
                seg_row[o] = rk;
                seg_label[o] = rk < 0 ? -1 : (rk < Kact ? rk : Kact);        // add_item's clamp (kmeans_components.py:103-106)
                seg_score[o] = id >= 0 ? cand.s[id] : NEG_INF_D;
            }
            ns += __popcll(mask);
            if (mask) start = c0 + 64 - __clzll((long long)mask);
        }
        for (int j = ns + lane; j < NM; j += 64) {         // the rest of the row: no segment
            seg_embed[row + j] = -1;
            seg_row[row + j] = -1;
            seg_label[row + j] = -1;
            seg_score[row + j] = NEG_INF_D;
        }
        for (int j = lane; j < NM; j += 64) boundaries[row + j] = j < N ? l_bnd[j] : (uint8_t)0;
        if (lane == 0) {
            n_seg[u] = ns;
            objective[u] = total;
        }
    }
}

extern "C" {

int32_t segk_kmd_decode(segk_ctx *ctx, const segk_corpus *cq, const segk_kmeans *m, const segk_cand *cand, int32_t n_slices_min,
                        int32_t n_slices_max, double wip, uint8_t *boundaries, int32_t *seg_embed, int32_t *seg_row,
                        int32_t *seg_label, double *seg_score, int32_t *n_seg, double *objective, void *stream)
{
    SEGK_REQUIRE(ctx && cq && m, "NULL context / held-out corpus / model");
    SEGK_REQUIRE(n_slices_min == 0 || n_slices_min == 1,
                 "n_slices_min must be 0 or 1 (>= 2 crashes in the reference, SURVEY 8(c))");
    SEGK_REQUIRE(n_slices_max >= 0, "n_slices_max must be >= 0 (0: no window)");
    SEGK_REQUIRE(cq->n_utt >= 0, "n_utt");
    if (cq->n_utt == 0) return SEGK_OK;
    SEGK_REQUIRE(cq->N_max > 0 && cq->lengths && cq->vec_ids && cq->durations, "held-out corpus without span tables");
    SEGK_REQUIRE(m->K && cand && cand->k && cand->s, "model without K / candidates without k, s");
    SEGK_REQUIRE(boundaries && seg_embed && seg_row && seg_label && seg_score && n_seg && objective, "NULL argument");
    const int NM = cq->N_max;
    const int Wc = (n_slices_max > 0 && n_slices_max < NM) ? n_slices_max : NM;
    const bool fast = n_slices_max >= 1 && n_slices_max <= 8 && NM <= 64;
    SEGK_REQUIRE((int64_t)NM * Wc < ((int64_t)1 << 28), "band of spans");
    const size_t wave_bytes = kmd_lds(NM, Wc, fast);
    if (wave_bytes > KMD_LDS_MAX) {
        segk_set_error("segk_kmd_decode: the band of %d x %d spans of the longest held-out utterance needs %zu bytes of LDS, a "
                       "workgroup has %d: set n_slices_max or split the longest utterances", NM, Wc, wave_bytes, KMD_LDS_MAX);
        return SEGK_ERR_UNSUPPORTED;
    }
    int waves = 4;
    while (waves > 1 && waves * wave_bytes > 64 * 1024) waves >>= 1;
    const size_t lds = waves * wave_bytes;
    const dim3 grid((unsigned)((cq->n_utt + waves - 1) / waves)), block(64 * waves);
    hipStream_t st = (hipStream_t)stream;
    if (fast) {
        SEGK_CHECK_HIP(segk_dyn_lds((const void *)k_kmd_decode<true>, lds));
        hipLaunchKernelGGL((k_kmd_decode<true>), grid, block, lds, st, *cq, m->K, n_slices_max, wip, *cand, boundaries, seg_embed,
                           seg_row, seg_label, seg_score, n_seg, objective, NM * Wc, (int)wave_bytes);
    } else {
        SEGK_CHECK_HIP(segk_dyn_lds((const void *)k_kmd_decode<false>, lds));
        hipLaunchKernelGGL((k_kmd_decode<false>), grid, block, lds, st, *cq, m->K, n_slices_max, wip, *cand, boundaries, seg_embed,
                           seg_row, seg_label, seg_score, n_seg, objective, NM * Wc, (int)wave_bytes);
    }
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

}  // extern "C"
