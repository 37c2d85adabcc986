// segk_fbitems.hip -- the item step of the batch-synchronous sweep of the stand-alone FBGMM (FBGMM.gibbs_sample(sync="batch"),
// fbgmm.py:288-463 as a blocked sampler; specification tests/fbgmm_items.py on oracle/np_fbgmm_batch.py).  The sweep is the
// unigram segmenter's with "utterance" read as "item": the statistics come from the segmenter's own entry points
// (segk_fbb_partials / _prepare / _canonical on a corpus of one-landmark utterances: new_tok[i] = i, n_new[i] = does item i hold
// a slot), and this unit adds what a segmenter step does with three kernels for one token each:
//
//   k_fbi_assign<XT, COV>   a workgroup takes a tile of FBI_T = 64 items of one (slice, block) cell: one lane per item, eight
//                           waves over the slots.  The slots are walked FBI_KC = 16 at a time, their (mean, q) staged in LDS once
//                           per tile and read as broadcasts; per (item, slot) the operations are those of fbb_accumulate_rows
//                           / fbb_slot_ll (segk_fbbatch.hip), dimensions in increasing order, so the likelihoods are the bits
//                           k_fbb_assign forms for the same row and statistics.  The tile's logits [64][K_max] stay in LDS
//                           where they fit (FBI_LDS_MAX) and go to a workspace of the context otherwise; then one wave per
//                           item: prior term, softmax, annealing and draw (fbb_draw_row: k_fbb_assign's statements).
//   cov_type 2              the likelihoods of the block's items are formed by k_fcb_token_ll (segk_fullcov.hip: one slot's
//                           packed triangle staged per 256 items) into its context table; k_fbi_assign<XT, 2> is the draw half
//                           reading that table.
// No grid barrier, no spin loop, no cooperative launch, no atomics: a plain grid over the tiles.
#include "segk_fb_common.h"
#include "segk_fbb_dev.h"

#define FBI_T 64            // items per tile: a lane each
#define FBI_NT 512          // threads: eight waves over the slots (likelihoods), over the items (draws)
#define FBI_KW 2            // slots a wave accumulates side by side (one read of x per dimension for the two)
#define FBI_KC (FBI_KW * (FBI_NT / 64))      // slots staged per pass
// a workgroup's LDS with the logits in it at most; beyond it the logits live in the context's workspace
#define FBI_LDS_MAX (144 * 1024)
// the workspace holds the logits of the tiles of ONE launch and never more than FBI_Z_MIB MiB (or one tile's, should that be
// more: 4 MiB at K_max = 8192): a block of more tiles is walked in several launches.  SEGK_FBI_Z_MIB is a launch-plan switch
// like SEGK_FBB_SORT -- another bound, the same results (the tests walk a block in several launches with it)
#define FBI_Z_MIB 64

static __host__ __device__ __forceinline__ size_t fbi_stage_doubles(int D) { return (size_t)FBI_T * D + 2 * (size_t)FBI_KC * D; }

// n_new[i] = 1 for every item of block b of the local slices (consider_unassigned with cov_type 2: k_fcb_token_ll evaluates the
// tokens n_new names)
__global__ __launch_bounds__(256) void k_fbi_mark(segk_fbatch bt, int s_lo, int b, int32_t *n_new)
{
    const int slice = s_lo + blockIdx.y;
    const int u0 = bt.utt_range[(slice * bt.n_blocks + b) * 2], u1 = bt.utt_range[(slice * bt.n_blocks + b) * 2 + 1];
    const int i = u0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (i < u1) n_new[i] = 1;
}

template <typename XT, int COV>
__global__ __launch_bounds__(FBI_NT) void k_fbi_assign(segk_corpus c, segk_fbgmm f, segk_fbatch bt, FbbMap map, int wg0, int b,
                                                      uint64_t sweep, double prior_alpha, double anneal_temp, int consider_unassigned,
                                                      int32_t *n_new, double *zbuf, const double *fc_ll, int fc_ucap,
                                                      double *probe_ll, int64_t probe_ld)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int D = c.D, KM = f.K_max, tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);        // (wave-uniform, and known to be)
    int s, idx;
    if (!fbb_locate(map, wg0 + blockIdx.x, &s, &idx)) return;
    const int slice = map.lo[s];
    const int u0 = bt.utt_range[(slice * bt.n_blocks + b) * 2], u1 = bt.utt_range[(slice * bt.n_blocks + b) * 2 + 1];
    const int i0 = u0 + idx * FBI_T;                        // the tile's first item
    const int nr = u1 - i0 < FBI_T ? u1 - i0 : FBI_T;       // (>= 1: the host counts the tiles from the same ranges)
    double *ll;                                             // [FBI_T][K_max] likelihood part of the logits, then the probabilities
    if constexpr (COV == 2) {
        // k_fcb_token_ll's table: row (local slice * u_cap + item of the cell), the row's prior predictive in the empty slots
        ll = const_cast<double *>(fc_ll) + ((int64_t)s * fc_ucap + (int64_t)idx * FBI_T) * KM;
    } else {
        double *xs = (double *)smem;                        // [D][FBI_T]: the lanes' rows side by side
        double *pm = xs + (size_t)FBI_T * D;                // [FBI_KC][D][2]: (mean, q) of the staged slots
        ll = zbuf ? zbuf + (int64_t)blockIdx.x * FBI_T * KM : pm + 2 * (size_t)FBI_KC * D;
        const XT *X = (const XT *)c.X;
        for (int j = tid; j < FBI_T * D; j += FBI_NT) {
            const int r = j / D, d = j - r * D;
            xs[d * FBI_T + r] = r < nr ? (double)X[(int64_t)(i0 + r) * c.ldx + d] : 0.0;
        }
        const bool valid = lane < nr;
        const double lp = valid ? bt.prior_rows[i0 + lane] : 0.0;       // an empty slot's likelihood: the row's prior predictive
        for (int k0 = 0; k0 < KM; k0 += FBI_KC) {
            __syncthreads();                                // (the rows are staged; the previous pass has read its parameters)
            for (int j = tid; j < FBI_KC * D; j += FBI_NT) {
                const int kk = j % FBI_KC, d = j / FBI_KC, k = k0 + kk;
                pm[((size_t)kk * D + d) * 2] = k < KM ? bt.mean_t[(int64_t)d * KM + k] : 0.0;
                pm[((size_t)kk * D + d) * 2 + 1] = k < KM ? bt.q_t[(int64_t)d * KM + k] : 0.0;
            }
            __syncthreads();
            const int kw = k0 + w * FBI_KW;                 // this wave's slots kw .. kw + FBI_KW - 1 (wave-uniform)
            bool occ[FBI_KW];
            double acc[FBI_KW];
            bool any = false;
#pragma unroll
            for (int j = 0; j < FBI_KW; j++) {
                occ[j] = kw + j < KM && bt.cnt[kw + j] > 0.0;
                acc[j] = 0.0;
                any = any || occ[j];
            }
            if (any) {
                const double *pw = pm + (size_t)(w * FBI_KW) * D * 2;
                for (int d = 0; d < D; d++) {
                    const double x = xs[d * FBI_T + lane];
#pragma unroll
                    for (int j = 0; j < FBI_KW; j++) {
                        if (!occ[j]) continue;
                        const double m = pw[((size_t)j * D + d) * 2], q = pw[((size_t)j * D + d) * 2 + 1];
                        const double delta = m - x;
                        if (COV == 0) acc[j] += (delta * delta) * q;
                        else acc[j] += log(1. + (delta * delta) * q);
                    }
                }
            }
            if (valid) {
#pragma unroll
                for (int j = 0; j < FBI_KW; j++) {
                    const int k = kw + j;
                    if (k >= KM) continue;
                    ll[(int64_t)lane * KM + k] = occ[j] ? bt.lconst[k] - bt.half[k] * acc[j] : lp;
                }
            }
        }
        __syncthreads();
    }
    if (probe_ll) {             // the likelihood part of the logits, as the draws below use it
        for (int j = tid; j < nr * KM; j += FBI_NT) {
            const int r = j / KM, k = j - r * KM;
            probe_ll[(int64_t)(i0 + r) * probe_ld + k] = ll[(int64_t)r * KM + k];
        }
        __syncthreads();
    }
    const double zc_empty = f.lms * log(prior_alpha / (double)KM);
    for (int r = w; r < nr; r += FBI_NT / 64) {             // a wave per item
        const int i = i0 + r;
        if (!consider_unassigned && bt.slot[i] < 0) continue;           // (wave-uniform) keeps -1 and contributes to nothing
        const int k = fbb_draw_row(f, bt, KM, prior_alpha, zc_empty, anneal_temp, ll + (int64_t)r * KM, sweep, (uint64_t)i, 1ull, lane);
        if (lane == 0) {
            bt.slot[i] = k;
            n_new[i] = 1;
        }
    }
}

extern "C" {

int32_t segk_fbi_assign(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, int32_t s_lo,
                        int32_t s_n, int32_t b, const int32_t *n_items, uint64_t sweep, double anneal_temp,
                        int32_t consider_unassigned, const int32_t *new_tok, int32_t *n_new, double *probe_ll, int64_t probe_ld,
                        void *stream)
{
    SEGK_REQUIRE(ctx && c && f && bt && n_items && new_tok && n_new, "NULL argument");
    if (f->lm_unigram) {
        segk_set_error("segk_fbi_assign: the stand-alone batch sweep takes no language model");
        return SEGK_ERR_UNSUPPORTED;
    }
    SEGK_REQUIRE(c->x_dtype == SEGK_F32 || c->x_dtype == SEGK_F64, "unsupported dtype");
    SEGK_REQUIRE(f->cov_type >= 0 && f->cov_type <= 2, "cov_type must be 0 (fixed), 1 (diag) or 2 (full)");
    SEGK_REQUIRE(!c->vec_ids && !c->band_ids && c->N_max == 1 && c->n_utt == c->n_emb,
                 "a corpus of items: one one-landmark utterance per row, no span tables");
    SEGK_REQUIRE(c->D > 0 && c->D <= 256, "batch mode supports D <= 256");
    SEGK_REQUIRE(f->K_max >= 1 && f->K_max <= 8192, "K_max");
    SEGK_REQUIRE(bt->n_slices >= 1 && bt->n_slices <= 16 && bt->n_blocks >= 1, "slices / blocks");
    SEGK_REQUIRE(s_lo >= 0 && s_n >= 1 && s_n <= 16 && s_lo + s_n <= bt->n_slices && b >= 0 && b < bt->n_blocks, "slice / block range");
    SEGK_REQUIRE(bt->prior_rows && bt->utt_range && bt->slot && bt->cnt && bt->mean_t && bt->q_t && bt->lconst && bt->half,
                 "batch state (prior_rows, ranges, slot, slot tables)");
    SEGK_REQUIRE(!probe_ll || probe_ld >= f->K_max, "probe leading dimension");
    if (f->cov_type == 2)
        if (int rc = segk_fcb_check(c, f, bt, "segk_fbi_assign")) return rc;
    FbbMap m;
    m.n = s_n;
    m.off[0] = 0;
    int most = 0;
    for (int s = 0; s < s_n; s++) {
        SEGK_REQUIRE(n_items[s] >= 0, "item counts");
        m.lo[s] = s_lo + s;
        m.off[s + 1] = m.off[s] + (n_items[s] + FBI_T - 1) / FBI_T;
        most = n_items[s] > most ? n_items[s] : most;
    }
    const int n_wg = m.off[s_n];
    if (n_wg == 0) return SEGK_OK;
    hipStream_t st = (hipStream_t)stream;
    const double *fc_ll = nullptr;
    int fc_ucap = 0;
    size_t lds = 0;
    int per_launch = n_wg;
    double *zbuf = nullptr;
    if (f->cov_type == 2) {
        if (consider_unassigned) {
            hipLaunchKernelGGL(k_fbi_mark, dim3((unsigned)((most + 255) / 256), (unsigned)s_n), dim3(256), 0, st, *bt, s_lo, b, n_new);
            SEGK_LAUNCH_CHECK();
        }
        if (int rc = segk_fcb_token_ll(ctx, c, f, bt, s_lo, s_n, b, n_items, new_tok, n_new, &fc_ll, &fc_ucap, stream)) return rc;
    } else {
        const size_t stage = fbi_stage_doubles(c->D) * sizeof(double), tile = (size_t)FBI_T * f->K_max * sizeof(double);
        SEGK_REQUIRE(stage <= FBI_LDS_MAX, "the rows and the staged slots of a tile do not fit in LDS");
        if (stage + tile <= FBI_LDS_MAX) {
            lds = stage + tile;
        } else {
            lds = stage;
            const int mib = segk_env_int("SEGK_FBI_Z_MIB", FBI_Z_MIB);
            const size_t cap = ((size_t)(mib > 0 ? mib : FBI_Z_MIB) << 20) / tile;
            per_launch = cap < 1 ? 1 : (cap < (size_t)n_wg ? (int)cap : n_wg);
            const int64_t need = (int64_t)per_launch * FBI_T * f->K_max;
            if (int rc = segk_ws_grow(ctx, &ctx->fbi_z, &ctx->fbi_z_n, need, (size_t)need * sizeof(double), st)) return rc;
            zbuf = ctx->fbi_z;
        }
    }
#define SEGK_FBI(XT, COV)                                                                                                       \
    do {                                                                                                                        \
        SEGK_CHECK_HIP(segk_dyn_lds((const void *)k_fbi_assign<XT, COV>, lds));                                                 \
        for (int wg0 = 0; wg0 < n_wg; wg0 += per_launch) {                                                                      \
            const int n = n_wg - wg0 < per_launch ? n_wg - wg0 : per_launch;                                                    \
            hipLaunchKernelGGL((k_fbi_assign<XT, COV>), dim3((unsigned)n), dim3(FBI_NT), lds, st, *c, *f, *bt, m, wg0, b, sweep, \
                               f->alpha, anneal_temp, consider_unassigned ? 1 : 0, n_new, zbuf, fc_ll, fc_ucap, probe_ll,       \
                               probe_ld);                                                                                       \
        }                                                                                                                       \
    } while (0)
    if (c->x_dtype == SEGK_F32) {
        if (f->cov_type == 0) SEGK_FBI(float, 0);
        else if (f->cov_type == 1) SEGK_FBI(float, 1);
        else SEGK_FBI(float, 2);
    } else {
        if (f->cov_type == 0) SEGK_FBI(double, 0);
        else if (f->cov_type == 1) SEGK_FBI(double, 1);
        else SEGK_FBI(double, 2);
    }
#undef SEGK_FBI
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

}  // extern "C"
