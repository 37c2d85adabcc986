// segk_fbb_dev.h -- what the batch sampler's translation units share (segk_fbbatch.hip; segk_fullcov.hip for the
// full-covariance forms of its kernels; segk_fbitems.hip for the stand-alone model's item step): the record of a (block,
// slice) cell, the workgroup -> (slice, index) map of a launch, the specification's balanced tree, the float32 Student-t
// term, the draw of one token's slot and its MAP counterpart.  Not part of the ABI.
#pragma once
#include "segk_internal.h"
#include "segk_fb_common.h"

// doubles of the partial sums of one (block, slice) cell: counts [K_max], sum x [K_max, D], then sum x^2 [K_max, D] or, with
// full-covariance components (cov_type 2), the lower triangle of sum outer(x, x) per slot, packed [K_max, D (D + 1) / 2] --
// entry (a, b), a >= b, at fbb_tri_index(D, a, b): the products are symmetric bit for bit
static __host__ __device__ __forceinline__ int fbb_tri(int D) { return D * (D + 1) / 2; }
static __host__ __device__ __forceinline__ int fbb_tri_index(int D, int a, int b) { return b * D - b * (b - 1) / 2 + (a - b); }
static __host__ __device__ __forceinline__ int64_t fbb_rec(const segk_fbgmm &f, int D)
{
    return f.cov_type == 2 ? (int64_t)f.K_max * (1 + D + fbb_tri(D)) : (int64_t)f.K_max * (2 * D + 1);
}

// which (slice, local index) a workgroup works on: `off` is the prefix of the per-slice counts
struct FbbMap {
    int n;
    int lo[16];
    int off[17];
};

static __device__ __forceinline__ bool fbb_locate(const FbbMap &m, int wg, int *slice, int *idx)
{
    for (int s = 0; s < m.n; s++)
        if (wg < m.off[s + 1]) {
            *slice = s;
            *idx = wg - m.off[s];
            return true;
        }
    return false;
}

// the pairing of oracle tree_sum: [(0+1), (2+3), ...], odd element carried
static __device__ __forceinline__ double fbb_tree(double *p, int n, int stride)
{
    while (n > 1) {
        const int h = n >> 1;
        for (int j = 0; j < h; j++) p[j * stride] = p[2 * j * stride] + p[(2 * j + 1) * stride];
        if (n & 1) p[h * stride] = p[(n - 1) * stride];
        n = (n + 1) >> 1;
    }
    return p[0];
}

// my[s * stride] = sum over the blocks bp != b of partials[(bp * S + s) * rec + off], in block order, for every slice s: the
// loads of eight slices x eight blocks are in flight together (k_fbb_prepare's own form of this is its `sum_slices`)
static __device__ __forceinline__ void fbb_sum_slices(const segk_fbatch &bt, int64_t rec, int64_t off, int b, double *my, int stride)
{
    const int S = bt.n_slices, B = bt.n_blocks;
    for (int s0 = 0; s0 < S; s0 += 8) {
        double a[8];
#pragma unroll
        for (int i = 0; i < 8; i++) a[i] = 0.0;
        for (int bp0 = 0; bp0 < B; bp0 += 8) {
            double v[8][8];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int sidx = s0 + i < S ? s0 + i : S - 1;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int bp = bp0 + j < B ? bp0 + j : B - 1;
                    v[i][j] = bt.partials[((int64_t)bp * S + sidx) * rec + off];
                }
            }
#pragma unroll
            for (int i = 0; i < 8; i++)
#pragma unroll
                for (int j = 0; j < 8; j++)
                    if (bp0 + j < B && bp0 + j != b) a[i] += v[i][j];
        }
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (s0 + i < S) my[(s0 + i) * stride] = a[i];
    }
}

// THE float32 Student-t term of one (row, slot, dimension) on the hardware logarithm (v_log_f32: log2; the caller multiplies
// the sum by ln 2): m = float(mean - centre), q = float(q), x = float(x - centre), the differences formed in fp64.  The one
// copy behind fbb_accumulate_rows32 (segk_fbbatch.hip: the segmenter's `score_precision="f32"` token likelihoods) and
// k_fbi_assign_diag32 (segk_fbitems.hip: the stand-alone model's), so the two routes cannot drift apart.
//
// log2(1 + e), e = delta^2 q, COMPENSATED: inside a slot of n_k items e is of the order of 1 / n_k, the sum
// u = 1 + e rounds away up to 2^-24 of it, and the slot's factor (v_N + 1) / 2 ~ n_k / 2 multiplies that back up -- an error of
// the likelihood that grows with the count whatever the data's scale.  c = e - (u - 1) is the part the addition dropped (both
// differences are exact for u < 2) and log2(1 + e) = log2(u) + c / (u ln 2) + O(c^2).  The factor 1 / u is left out, and the
// correction with it from u = 2 on: there c / u is at most 2^-24, below the last bit of a logarithm that is 1 or more, while c
// alone would grow with u.  For u < 2 the missing factor costs at most 2^-25 / ln 2 per term.  (The comparison against 2 and a
// select, both on inline constants: a clamp of c to +-2^-24 by v_med3_f32 wants two registers for its bounds, which the
// token kernels at their register limit do not have.)  The library is built without fast-math and with -ffp-contract=off
// (Makefile): nothing re-associates e - (u - 1) away.
#define FBB_LOG2E_F 1.4426950408889634f
static __device__ __forceinline__ float fbb_log2_1p32(float e)
{
    const float u = 1.f + e;
    const float c = u < 2.f ? e - (u - 1.f) : 0.f;
    return __builtin_fmaf(c, FBB_LOG2E_F, __builtin_amdgcn_logf(u));
}

// The same term on a PAIR of rows, for the packed float32 loops of k_fbb_score_diag32 and k_fbb_step_diag32 (segk_fbbatch.hip):
// d2 = delta^2 of the two rows, q2 = (q, q).  u = fma(d2, q2, 1) as those loops always formed it, and c = fma(d2, q2, 1 - u):
// the product unrounded less u - 1 (1 - u is exact) -- again what the addition dropped.  Three packed instructions and a
// compare and select per row more than log2(u) alone.
typedef float fbb_f32x2 __attribute__((ext_vector_type(2)));
static __device__ __forceinline__ fbb_f32x2 fbb_log2_1p32x2(fbb_f32x2 d2, fbb_f32x2 q2)
{
    const fbb_f32x2 one2 = {1.f, 1.f}, log2e2 = {FBB_LOG2E_F, FBB_LOG2E_F};
    const fbb_f32x2 u = __builtin_elementwise_fma(d2, q2, one2);
    const fbb_f32x2 c = __builtin_elementwise_fma(d2, q2, one2 - u);
    const fbb_f32x2 cc = {u.x < 2.f ? c.x : 0.f, u.y < 2.f ? c.y : 0.f};
    const fbb_f32x2 lg = {__builtin_amdgcn_logf(u.x), __builtin_amdgcn_logf(u.y)};                     // v_log_f32: log2
    return __builtin_elementwise_fma(cc, log2e2, lg);
}

static __device__ __forceinline__ float fbb_term32(float m, float q, float x)
{
    const float delta = m - x;
    return fbb_log2_1p32((delta * delta) * q);
}

// THE draw of one token's slot without a language model, by one wave (k_fbb_slots of segk_fbbatch.hip: a wave per token of an
// utterance; k_fbi_assign of segk_fbitems.hip: a wave per item of a tile): zr[k] holds the likelihood part of the logits of all
// K_max slots (LDS or memory; overwritten).  The prior's term lms log(alpha / K_max + n_k) (fbgmm.py:436-440), the softmax, the
// annealing (fbgmm.py:446-449) and the inverse-CDF walk on u01(seed, sweep, utt, j).  The sums keep the association of a
// block-wide sum at 256 threads (per wave of 64 consecutive slots a butterfly, the waves' results added in order: block_sum,
// as k_fbb_assign_lm uses it), so the probabilities -- and the draws -- are the bits a block-wide softmax of the same logits
// gives.  Result in all lanes.
static __device__ __forceinline__ int fbb_draw_row(const segk_fbgmm &f, const segk_fbatch &bt, int KM, double prior_alpha, double zc_empty,
                                                   double anneal_temp, double *zr, uint64_t sweep, uint64_t utt, uint64_t j, int lane)
{
    double mx = NEG_INF_D;
    for (int k = lane; k < KM; k += 64) {
        const double n = bt.cnt[k];
        const double v = (n > 0.0 ? f.lms * log(prior_alpha / (double)KM + n) : zc_empty) + zr[k];      // fbgmm.py:436-440
        zr[k] = v;
        mx = v > mx ? v : mx;
    }
    mx = fb_wave_max(mx, false);
    auto sum_exp = [&](double shift) -> double {       // sum_k exp(zr[k] - shift) in the order of block_sum at 256 threads
        double tot = 0.0;
        for (int cw = 0; cw < 4 && cw * 64 < KM; cw++) {
            double sv = 0.0;
            for (int k = cw * 64 + lane; k < KM; k += 256) sv += exp(zr[k] - shift);
            sv = fb_wave_sum(sv);
            tot = cw == 0 ? sv : tot + sv;
        }
        return tot;
    };
    double lse = log(sum_exp(mx)) + mx;
    if (anneal_temp != 1.0) {                           // fbgmm.py:446-449
        double mx2 = NEG_INF_D;
        for (int k = lane; k < KM; k += 64) {
            const double v = (1. / anneal_temp) * (zr[k] - lse);
            zr[k] = v;
            mx2 = v > mx2 ? v : mx2;
        }
        mx2 = fb_wave_max(mx2, false);
        lse = log(sum_exp(mx2)) + mx2;
    }
    for (int k = lane; k < KM; k += 64) zr[k] = exp(zr[k] - lse);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return fb_draw_chunked(zr, KM, segk_u01(bt.seed, sweep, utt, j), lane);
}

static __device__ __forceinline__ int fbb_wave_min_i32(int v)       // minimum over the 64 lanes, wave-uniform
{
    int o = __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false);
    v = o < v ? o : v;
    o = __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false);
    v = o < v ? o : v;
    o = __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false);
    v = o < v ? o : v;
    o = __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false);
    v = o < v ? o : v;
    const int r0 = __builtin_amdgcn_readlane(v, 0), r1 = __builtin_amdgcn_readlane(v, 16);
    const int r2 = __builtin_amdgcn_readlane(v, 32), r3 = __builtin_amdgcn_readlane(v, 48);
    const int a = r1 < r0 ? r1 : r0, c = r3 < r2 ? r3 : r2;
    return c < a ? c : a;
}

// THE MAP slot of one token, by one wave (k_fbb_slots<.., MAP> of segk_fbbatch.hip; the MAP halves of k_fbi_assign and
// k_fbi_assign_diag32 of segk_fbitems.hip): the first index of the maximum of z_k = pz[k] + zr[k] over the K_max slots, where
// pz[k] = log(alpha / K_max + n_k) (fbgmm.py:475-479: no lms) and zr the likelihood part of the logits (read only).  A per-lane
// (value, index) over k = lane, lane + 64, ... with strict >, the wave's maximum by DPP, then the lowest index among the lanes
// that hold it.  All empty slots of a token carry one value, so the first of them wins a tie among them without being treated
// apart.  Result in all lanes.
static __device__ __forceinline__ int fbb_map_row(const double *pz, const double *zr, int KM, int lane)
{
    double best = NEG_INF_D;
    int bk = KM;
    for (int kk = lane; kk < KM; kk += 64) {
        const double z = pz[kk] + zr[kk];
        if (z > best) { best = z; bk = kk; }
    }
    const double m = fb_wave_max(best, false);
    const int k = fbb_wave_min_i32(best == m ? bk : KM);
    return k < KM ? k : 0;
}

// segk_fullcov.hip: the cov_type 2 forms of the segk_fbb_* entry points a unigram step uses (arguments checked by the callers
// in segk_fbbatch.hip, which also bucket the block's tokens by slot -- k_fbb_sort -- for the partial sums)
int segk_fcb_check(const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, const char *who);
int segk_fcb_partials(const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, int s_lo, int s_n, int b,
                      const int32_t *sorted, int64_t sorted_stride, const int32_t *koff, void *stream);
int segk_fcb_prepare(const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, int b, void *stream);
int segk_fcb_score(const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, int s_lo, int s_n, int b, const int32_t *n_rows,
                   double *score, void *stream);
// token likelihoods of the block's new segments into a table the context owns: row (local slice * *u_cap + utterance of the
// cell) * N_max + token, [K_max] each, the row's prior predictive in the empty slots (k_fbb_slots reads it)
int segk_fcb_token_ll(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, int s_lo, int s_n, int b,
                      const int32_t *n_utts, const int32_t *new_tok, const int32_t *n_new, const double **ll, int *u_cap,
                      void *stream);
// the prior predictive (`cached_log_prior`, :125-127) of rows that are not the model's: `c` a view of them (X, ldx, n_emb), written
// to out [c->n_emb] (segk_fbi_predict: the query rows; segk_fbb_prior_rows with cov_type 2 copies the TRAINING rows' cache)
int segk_fc_prior_rows_view(const segk_corpus *c, const segk_fbgmm *f, double *out, void *stream);
