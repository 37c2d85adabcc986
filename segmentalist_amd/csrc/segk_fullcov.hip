// segk_fullcov.hip -- gfx950 kernels of the full-covariance FBGMM components (segk_fbgmm, cov_type 2):
// the device image of `GaussianComponents` (gaussian_components.py) and the item loops of the stand-alone
// `FBGMM` (fbgmm.py:256-285, 352-494) over it.  fp64 throughout, X float32 or float64.
//
// Per component k: stat_a[k] = m_N_numerators (D), stat_b[k] = S_N_partials (D x D, row-major), counts[k].
// After every add and delete the derived values are recomputed from scratch (:319-331),
//     covar = (k_N + 1) / (k_N (v_N - D + 1)) (S_N_partial - k_N m_N m_N'),
// kept as the lower Cholesky factor L of covar where the reference keeps the inverse:
//     pred[k][j * D + d] = L[d][j]  (d >= j; zero above the diagonal) -- column j of L is contiguous, it is
//                                   what step j of a forward substitution reads, one element per lane
//     log_prod[k]        = logdet covar = 2 sum log L_dd
//     kconst[k]          = lgamma((v + D) / 2) - lgamma(v / 2) - D/2 log v - D/2 log pi,  v = v_N - D + 1
// and the predictive (:334-344) is kconst - logdet / 2 - (v + D) / 2 log(1 + |L^-1 delta|^2 / v).
// prior_c [D * D + n_emb + 1] is written by segk_fbgmm_init_stats: the factor of the prior's covar (same
// layout), the prior predictive of every row (`cached_log_prior`, :125-127), one status word (FC_STATUS_*).
//
//   k_fc_init / k_fc_prior_rows   __init__ (:95-127)
//   k_fc_update                   add_item / del_item / del_component (:154-205)
//   k_fc_del_utt                  del_item over an utterance's segments (unigram_acoustic_wordseg.py:270-273)
//   k_fc_score                    FBGMM.log_marg_i (fbgmm.py:256-285), a workgroup per row
//   k_fc_span_terms / _span_lse   the same for a long list of rows (an utterance's triangle), a lane per row
//   k_fc_pred_vector              log_post_pred / log_prior (:207-251)
//   k_fc_assign                   gibbs_sample_inside_loop_i / map_assign_i (fbgmm.py:422-494)
//   k_fc_gibbs_items              the inner loop of FBGMM.gibbs_sample (fbgmm.py:352-405)
//
// Every kernel is a plain grid of independent workgroups or a single workgroup; D <= 64 (one lane per
// dimension in the substitution, a D x D fp64 matrix in LDS for the factorisation).
#include "segk_internal.h"
#include "segk_fb_common.h"
#include "segk_fbb_dev.h"

#define FC_DMAX 64
#define FC_NT 512                      // threads of every kernel of this unit
#define FC_STATUS_PIVOT 32             // a refresh met a non-positive or non-finite pivot: the component kept its previous factor
#define FC_STATUS_INDEX 64             // add_item / del_component named a component beyond K

static __device__ __forceinline__ int32_t *fc_status(const segk_corpus &c, const segk_fbgmm &f)
{
    return (int32_t *)(f.prior_c + (int64_t)c.D * c.D + c.n_emb);
}
static __device__ __forceinline__ const double *fc_prior_rows(const segk_corpus &c, const segk_fbgmm &f)
{
    return f.prior_c + (int64_t)c.D * c.D;
}

// x-independent constant of the Student-t with v degrees of freedom in D dimensions (:340-341; the reference
// reads lgamma(n / 2) and log(n) from tables indexed by n)
static __device__ double fc_const(int D, double v)
{
    return lgamma((v + (double)D) / 2.) - lgamma(v / 2.) - (double)D / 2. * log(v) - (double)D / 2. * LOG_PI;
}

// the products of np.outer(X[i], X[i]) as the reference caches them (:116-118): in the dtype of X, then widened
template <typename XT>
static __device__ __forceinline__ double fc_xprod(XT a, XT b)
{
    XT q = a * b;
    return (double)q;
}

// LDS of the single-workgroup kernels
struct FcLds {
    double *z;          // [K_max] logits
    double *red;        // [16]
    double *A;          // [D * D] the matrix being factored, column j contiguous: A[j * D + d]
    double *diag;       // [D] L_jj
    double *mN;         // [D]
    void *xs;           // [D] the row, in its own dtype
    int *ctl;           // [16] the workgroup's scalars: K, scratch of del_item, drawn component, old component
    double *dctl;       // [4] cached logdet, constant, count (as int64) of the old component
};
// (all of it in the dynamic region: static __shared__ variables in front of it would shift its base off 16 bytes)
#define FC_SHK 0
#define FC_SHI 1
#define FC_SHKNEW 3
#define FC_SHKOLD 4

// Right-looking Cholesky of the D x D matrix in A (lower triangle used; A[j * D + d], d >= j), in place, by the
// whole workgroup: D steps of pivot, column scale, trailing update.  The diagonal of L goes to diag[] (A's own
// diagonal keeps the pivots).  Returns false -- the same in every thread -- at the first pivot that is not a
// positive finite number; A is then half factored and must not be used.
static __device__ bool fc_cholesky(double *A, double *diag, int D)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    __syncthreads();
    for (int j = 0; j < D; j++) {
        const double p = A[j * D + j];                     // final since the barrier that ended step j - 1
        if (!(p > 0.0) || !(p < __builtin_huge_val())) return false;
        const double ljj = sqrt(p);
        const int m = D - 1 - j;
        for (int i = tid; i < m; i += nt) A[j * D + j + 1 + i] /= ljj;
        if (tid == 0) diag[j] = ljj;
        __syncthreads();
        // trailing update: a wave per column b, a lane per row a (D <= 64): column b and column j contiguous over the lanes
        const int a = j + 1 + (tid & 63);
        if (a < D) {
            const double la = A[j * D + a];
            for (int b = j + 1 + (tid >> 6); b <= a; b += nt >> 6) A[b * D + a] -= la * A[j * D + b];
        }
        __syncthreads();
    }
    return true;
}

// Derived values of component k from its statistics in global memory (:319-331): covar into LDS, factored, then L,
// logdet and the constant written.  A failed factorisation sets FC_STATUS_PIVOT and leaves pred / log_prod as
// they were.
static __device__ void fc_refresh(const segk_corpus &c, const segk_fbgmm &f, int k, const FcLds &S)
{
    const int tid = threadIdx.x, nt = blockDim.x, D = c.D;
    const double cnt = (double)f.counts[k];
    const double k_N = f.k_0 + cnt, v_N = f.v_0 + cnt;
    const double scale = (k_N + 1.) / (k_N * (v_N - (double)D + 1.));
    __syncthreads();
    for (int d = tid; d < D; d += nt) S.mN[d] = f.stat_a[(int64_t)k * D + d] / k_N;
    __syncthreads();
    const double *sb = f.stat_b + (int64_t)k * D * D;
    for (int i = tid; i < D * D; i += nt) {
        const int j = i / D, d = i - j * D;
        S.A[i] = scale * (sb[i] - k_N * (S.mN[d] * S.mN[j]));        // (S_N_partials is symmetric)
    }
    const bool ok = fc_cholesky(S.A, S.diag, D);
    if (!ok) {
        if (tid == 0) atomicOr(fc_status(c, f), FC_STATUS_PIVOT);
        __syncthreads();
        return;
    }
    double *pp = f.pred + (int64_t)k * D * D;
    for (int i = tid; i < D * D; i += nt) {
        const int j = i / D, d = i - j * D;
        pp[i] = d > j ? S.A[i] : (d == j ? S.diag[j] : 0.0);
    }
    const double part = tid < D ? log(S.diag[tid]) : 0.0;
    const double tot = block_sum(part, S.red);
    if (tid == 0) {
        f.log_prod[k] = 2. * tot;
        f.kconst[k] = fc_const(D, v_N - (double)D + 1.);
    }
    __syncthreads();
}

template <typename XT>
static __device__ void fc_load_row(const segk_corpus &c, int64_t e, const FcLds &S)
{
    __syncthreads();
    for (int d = threadIdx.x; d < c.D; d += blockDim.x) ((XT *)S.xs)[d] = ((const XT *)c.X)[e * c.ldx + d];
    __syncthreads();
}

// add_item(e, k) (:154-169); the row is in S.xs
template <typename XT>
static __device__ void fc_add_item(const segk_corpus &c, const segk_fbgmm &f, int64_t e, int k, int *shK, const FcLds &S)
{
    const int tid = threadIdx.x, nt = blockDim.x, D = c.D;
    const XT *x = (const XT *)S.xs;
    __syncthreads();
    const bool is_new = k == *shK;
    __syncthreads();
    if (tid == 0 && is_new) *shK = k + 1;
    double *sa = f.stat_a + (int64_t)k * D, *sb = f.stat_b + (int64_t)k * D * D;
    for (int i = tid; i < D * D; i += nt) {
        const int a = i / D, b = i - a * D;
        double s = is_new ? f.prior_a[i] + f.k_0 * (f.prior_b[a] * f.prior_b[b]) : sb[i];
        sb[i] = s + fc_xprod<XT>(x[a], x[b]);
    }
    for (int d = tid; d < D; d += nt) {
        double a = is_new ? f.k_0 * f.prior_b[d] : sa[d];
        sa[d] = a + (double)x[d];
    }
    if (tid == 0) {
        f.counts[k] += 1;
        f.assignments[e] = k;
    }
    __syncthreads();
    fc_refresh(c, f, k, S);
}

// del_component(k) (:188-205): swap-last compaction; *shK already decremented
static __device__ void fc_del_component(const segk_corpus &c, const segk_fbgmm &f, int k, int *shK)
{
    const int tid = threadIdx.x, nt = blockDim.x, D = c.D;
    __syncthreads();
    const int K = *shK;
    const int64_t DD = (int64_t)D * D;
    if (k != K) {
        for (int d = tid; d < D; d += nt) f.stat_a[(int64_t)k * D + d] = f.stat_a[(int64_t)K * D + d];
        for (int i = tid; i < D * D; i += nt) {
            f.stat_b[k * DD + i] = f.stat_b[K * DD + i];
            f.pred[k * DD + i] = f.pred[K * DD + i];
        }
        for (int64_t e = tid; e < c.n_emb; e += nt)
            if (f.assignments[e] == K) f.assignments[e] = k;
    }
    __syncthreads();
    for (int d = tid; d < D; d += nt) f.stat_a[(int64_t)K * D + d] = 0.0;
    for (int i = tid; i < D * D; i += nt) {
        f.stat_b[K * DD + i] = 0.0;
        f.pred[K * DD + i] = 0.0;
    }
    if (tid == 0) {
        if (k != K) {
            f.log_prod[k] = f.log_prod[K];
            f.kconst[k] = f.kconst[K];
            f.counts[k] = f.counts[K];
        }
        f.log_prod[K] = 0.0;
        f.kconst[K] = 0.0;
        f.counts[K] = 0;
    }
    __syncthreads();
}

// del_item(e) (:171-186); the row is in S.xs
template <typename XT>
static __device__ void fc_del_item(const segk_corpus &c, const segk_fbgmm &f, int64_t e, int *shK, int *sh_i, const FcLds &S)
{
    const int tid = threadIdx.x, nt = blockDim.x, D = c.D;
    const XT *x = (const XT *)S.xs;
    __syncthreads();
    if (tid == 0) {
        const int k = f.assignments[e];
        int emptied = 0;
        if (k != -1) {
            f.counts[k] -= 1;
            f.assignments[e] = -1;
            emptied = f.counts[k] == 0;
            if (emptied) *shK = *shK - 1;
        }
        sh_i[0] = k;
        sh_i[1] = emptied;
    }
    __syncthreads();
    const int k = sh_i[0], emptied = sh_i[1];
    __syncthreads();                                        // sh_i is rewritten by the next call
    if (k == -1) return;
    if (emptied) {
        fc_del_component(c, f, k, shK);
        return;
    }
    double *sa = f.stat_a + (int64_t)k * D, *sb = f.stat_b + (int64_t)k * D * D;
    for (int i = tid; i < D * D; i += nt) {
        const int a = i / D, b = i - a * D;
        sb[i] -= fc_xprod<XT>(x[a], x[b]);
    }
    for (int d = tid; d < D; d += nt) sa[d] -= (double)x[d];
    __syncthreads();
    fc_refresh(c, f, k, S);
}

// |L^-1 delta|^2 by one wave, lane d holding delta_d (zero in the lanes d >= D): D steps of forward substitution,
// each y_j = delta_j / L_jj broadcast and taken off the lanes below.  Lt: the factor, column j at Lt[j * D].
// The result is the same in every lane.
static __device__ double fc_mahalanobis(const double *Lt, double delta, int D, int lane)
{
    // Eight columns are fetched together and their reciprocal pivots formed before the steps that use them: the chain from
    // one step to the next is then two lane reads, two multiplications and a subtraction, not a load and a division.
    double y = 0.0;
    for (int j0 = 0; j0 < D; j0 += 8) {
        double l[8], r[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int j = j0 + q;
            l[q] = (j < D && lane >= j && lane < D) ? Lt[j * D + lane] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 8; q++) r[q] = 1. / fb_readlane(l[q], j0 + q < D ? j0 + q : 0);
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int j = j0 + q;
            if (j < D) {                                        // (wave-uniform)
                const double yj = fb_readlane(delta, j) * r[q];
                delta -= l[q] * yj;                             // (the lanes above j see l = 0)
                if (lane == j) y = yj;
            }
        }
    }
    return fb_wave_sum(lane < D ? y * y : 0.0);
}

// log_post_pred_k of the row in S.xs under component k (:216-226), by one wave
template <typename XT>
static __device__ double fc_post_pred(const segk_corpus &c, const segk_fbgmm &f, int k, const XT *x, int lane)
{
    const int D = c.D;
    const double cnt = (double)f.counts[k];
    const double k_N = f.k_0 + cnt, v = f.v_0 + cnt - (double)D + 1.;
    const double delta = lane < D ? (double)x[lane] - f.stat_a[(int64_t)k * D + lane] / k_N : 0.0;
    const double s = fc_mahalanobis(f.pred + (int64_t)k * D * D, delta, D, lane);
    return f.kconst[k] - 0.5 * f.log_prod[k] - (v + (double)D) / 2. * log(1. + 1. / v * s);
}

// log_prior of the row x (:207-214), by one wave; kconst[K_max] holds the constant with the prior's -logdet / 2
template <typename XT>
static __device__ double fc_prior_pred(const segk_corpus &c, const segk_fbgmm &f, const XT *x, int lane)
{
    const int D = c.D;
    const double v = f.v_0 - (double)D + 1.;
    const double delta = lane < D ? (double)x[lane] - f.prior_b[lane] : 0.0;
    const double s = fc_mahalanobis(f.prior_c, delta, D, lane);
    return f.kconst[f.K_max] - (v + (double)D) / 2. * log(1. + 1. / v * s);
}

// logits z[k], k < K_max, of row e (in S.xs): assignment prior by `mode` (0 log_marg_i fbgmm.py:268-272, 1
// gibbs_sample_inside_loop_i :436-440, 2 map_assign_i :475-479) plus log_post_pred (k < K) or the row's cached prior
// predictive (k >= K).  The workgroup's waves share the components.
template <typename XT>
static __device__ void fc_logits(const segk_corpus &c, const segk_fbgmm &f, int64_t e, int mode, int K, const FcLds &S)
{
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, w = tid >> 6, nw = nt >> 6;
    const int KM = f.K_max;
    double total = 0.0;
    if (mode == 0) {
        double csum = 0.0;
        for (int k = tid; k < KM; k += nt) csum += (double)f.counts[k];
        total = block_sum(csum, S.red);                    // exact: integer-valued
    }
    __syncthreads();
    const double lprior = fc_prior_rows(c, f)[e];
    for (int k = w; k < K; k += nw) {
        const double pk = fc_post_pred<XT>(c, f, k, (const XT *)S.xs, lane);
        if (lane == 0) S.z[k] = pk;
    }
    __syncthreads();
    for (int k = tid; k < KM; k += nt) {
        const double lc = log(f.alpha / (double)KM + (double)f.counts[k]);
        double v;
        if (mode == 0) v = f.lms * (lc - log(total + f.alpha));
        else if (mode == 1) v = f.lms * lc;
        else v = lc;
        S.z[k] = v + (k < K ? S.z[k] : lprior);
    }
    __syncthreads();
}

static __device__ FcLds fc_carve(char *smem, int K_max, int D, char **end)
{
    FcLds S;
    S.z = (double *)smem;
    S.red = S.z + ((K_max + 1) & ~1);
    S.A = S.red + 16;
    S.diag = S.A + D * D;
    S.mN = S.diag + D;
    S.xs = (void *)(S.mN + D);
    S.ctl = (int *)((double *)S.xs + D);
    S.dctl = (double *)(S.ctl + 16);
    *end = (char *)(S.dctl + 4);
    return S;
}
static size_t fc_lds_bytes(int K_max, int D) { return (size_t)(((K_max + 1) & ~1) + 16 + D * D + 3 * D + 8 + 4) * sizeof(double); }

// ---------------------------------------------------------------------------------------
// __init__ (:95-127).  Workgroup k < K_max: add_item(i, k) for the rows i of component k ascending -- the
// statistics accumulated in that order, one refresh at the end (the factor after the last add is what the
// reference holds).  Workgroup K_max: the prior's factor and constant.
// ---------------------------------------------------------------------------------------
template <typename XT>
__global__ __launch_bounds__(FC_NT) void k_fc_init(segk_corpus c, segk_fbgmm f, const int32_t *blk_lo, int n_blocks,
                                                  const int32_t *sorted, const int32_t *koff)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *end;
    const FcLds S = fc_carve(smem, f.K_max, c.D, &end);
    const int tid = threadIdx.x, nt = blockDim.x, D = c.D, k = blockIdx.x;
    double *pc = const_cast<double *>(f.prior_c);
    if (k == f.K_max) {
        const double scale = (f.k_0 + 1.) / (f.k_0 * (f.v_0 - (double)D + 1.));
        for (int i = tid; i < D * D; i += nt) S.A[i] = scale * f.prior_a[i];
        const bool ok = fc_cholesky(S.A, S.diag, D);
        if (!ok) {
            if (tid == 0) atomicOr(fc_status(c, f), FC_STATUS_PIVOT);
            return;
        }
        for (int i = tid; i < D * D; i += nt) {
            const int j = i / D, d = i - j * D;
            pc[i] = d > j ? S.A[i] : (d == j ? S.diag[j] : 0.0);
        }
        const double tot = block_sum(tid < D ? log(S.diag[tid]) : 0.0, S.red);
        if (tid == 0) f.kconst[k] = fc_const(D, f.v_0 - (double)D + 1.) - 0.5 * (2. * tot);
        return;
    }
    const XT *X = (const XT *)c.X;
    // every thread owns the entries tid, tid + nt, ... of S_N_partials (at most FC_DMAX^2 / FC_NT = 8) and, below D,
    // one of m_N_numerators; the rows are walked in order by all of them
    constexpr int PER = FC_DMAX * FC_DMAX / FC_NT;
    double acc[PER], am = 0.0;
    int ia[PER], ib[PER];
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int i = tid + q * nt;
        acc[q] = 0.0;
        ia[q] = ib[q] = 0;
        if (i < D * D) {
            ia[q] = i / D;
            ib[q] = i - ia[q] * D;
            acc[q] = f.prior_a[i] + f.k_0 * (f.prior_b[ia[q]] * f.prior_b[ib[q]]);
        }
    }
    if (tid < D) am = f.k_0 * f.prior_b[tid];
    int64_t n = 0;
    for (int bb = 0; bb < n_blocks; bb++) {
        const int32_t *ko = koff + (int64_t)bb * (f.K_max + 1);
        const int64_t p0 = blk_lo[bb];
        for (int q = ko[k]; q < ko[k + 1]; q++) {
            const XT *x = X + (p0 + sorted[p0 + q]) * c.ldx;
            n++;
#pragma unroll
            for (int r = 0; r < PER; r++)
                if (tid + r * nt < D * D) acc[r] += fc_xprod<XT>(x[ia[r]], x[ib[r]]);
            if (tid < D) am += (double)x[tid];
        }
    }
    const int64_t DD = (int64_t)D * D;
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int i = tid + q * nt;
        if (i < D * D) {
            f.stat_b[k * DD + i] = n ? acc[q] : 0.0;
            f.pred[k * DD + i] = 0.0;
        }
    }
    if (tid < D) f.stat_a[(int64_t)k * D + tid] = n ? am : 0.0;
    if (tid == 0) {
        f.counts[k] = n;
        f.log_prod[k] = 0.0;
        f.kconst[k] = 0.0;
        if (n) atomicMax(f.K, k + 1);
    }
    __syncthreads();
    if (n) fc_refresh(c, f, k, S);
}

// cached_log_prior (:125-127): one wave per row
template <typename XT>
__global__ __launch_bounds__(256) void k_fc_prior_rows(segk_corpus c, segk_fbgmm f)
{
    const int64_t e = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (e >= c.n_emb) return;
    const double v = fc_prior_pred<XT>(c, f, (const XT *)c.X + e * c.ldx, lane);
    if (lane == 0) const_cast<double *>(f.prior_c)[(int64_t)c.D * c.D + e] = v;
}

// ... of rows that are not the model's (segk_fbi_predict: the query rows as a view `c` -- X, ldx, n_emb theirs --, written to
// `out`): the arithmetic of k_fc_prior_rows.  The view's n_emb is not the model's, so nothing here may derive an address
// inside prior_c from it (fc_status, fc_prior_rows): fc_prior_pred reads c.D alone
template <typename XT>
__global__ __launch_bounds__(256) void k_fc_prior_rows_view(segk_corpus c, segk_fbgmm f, double *out)
{
    const int64_t e = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (e >= c.n_emb) return;
    const double v = fc_prior_pred<XT>(c, f, (const XT *)c.X + e * c.ldx, lane);
    if (lane == 0) out[e] = v;
}

// op 1: add_item(item, k)   op 2: del_item(item)   op 4: del_component(k)
template <typename XT>
__global__ __launch_bounds__(FC_NT) void k_fc_update(segk_corpus c, segk_fbgmm f, int op, int64_t item, int k_item)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *end;
    const FcLds S = fc_carve(smem, f.K_max, c.D, &end);
    int &shK = S.ctl[FC_SHK];
    int *sh_i = S.ctl + FC_SHI;
    if (threadIdx.x == 0) shK = *f.K;
    __syncthreads();
    const int K = shK;
    if (op == 1) {
        if (k_item < 0 || k_item > K || k_item >= f.K_max) {
            if (threadIdx.x == 0) atomicOr(fc_status(c, f), FC_STATUS_INDEX);
            return;
        }
        fc_load_row<XT>(c, item, S);
        fc_add_item<XT>(c, f, item, k_item, &shK, S);
    } else if (op == 2) {
        fc_load_row<XT>(c, item, S);
        fc_del_item<XT>(c, f, item, &shK, sh_i, S);
    } else {
        if (k_item < 0 || k_item >= K) {
            if (threadIdx.x == 0) atomicOr(fc_status(c, f), FC_STATUS_INDEX);
            return;
        }
        __syncthreads();
        if (threadIdx.x == 0) shK = K - 1;
        fc_del_component(c, f, k_item, &shK);
    }
    __syncthreads();
    if (threadIdx.x == 0) *f.K = shK;
}

// op 0: del_item for every segment of the current segmentation of utterance `utt`, in the reference's order
// (unigram_acoustic_wordseg.py:270-273); one workgroup, every delete with its own refresh (the factor after the last
// delete of a component is a function of its statistics alone, so deferring the refreshes would give the same bits:
// not done, the bookkeeping across swap-last moves has not been shown to pay)
template <typename XT>
__global__ __launch_bounds__(FC_NT) void k_fc_del_utt(segk_corpus c, segk_fbgmm f, int utt, const uint8_t *boundaries)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *end;
    const FcLds S = fc_carve(smem, f.K_max, c.D, &end);
    int &shK = S.ctl[FC_SHK];
    int *sh_i = S.ctl + FC_SHI;
    if (threadIdx.x == 0) shK = *f.K;
    __syncthreads();
    const int N = c.lengths[utt];
    const int64_t triMax = (int64_t)c.N_max * (c.N_max + 1) / 2;
    const int32_t *vid = c.vec_ids + (int64_t)utt * triMax;
    const uint8_t *bnd = boundaries + (int64_t)utt * c.N_max;
    int jp = 0;
    for (int j = 0; j < N; j++) {
        if (bnd[j]) {                                       // uniform: every thread reads the same byte
            const int64_t id = vid[(j + 1) * j / 2 + jp];
            jp = j + 1;
            if (id >= 0 && id < c.n_emb) {
                fc_load_row<XT>(c, id, S);
                fc_del_item<XT>(c, f, id, &shK, sh_i, S);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) *f.K = shK;
}

// ---------------------------------------------------------------------------------------
// Span scores of many rows at once (the triangle of an utterance): a lane per row, a wave per (component, 64 rows).
// k_fc_score above spends, per (row, component), D dependent steps of lane reads on one useful multiply-add per lane;
// here the row's delta vector sits in the lane's registers, the component's factor (lower triangle, the diagonal slots
// holding the reciprocal pivots) and mean are staged once per workgroup in LDS and read as same-address broadcasts,
// and the substitution has no cross-lane traffic:  y_j = delta_j r_j,  s += y_j^2,  delta_d -= L_dj y_j (d > j),
// j ascending as in fc_mahalanobis.  DB: D rounded up to a multiple of 8 (compile-time bounds keep delta in registers;
// the padding is zeros).  The waves of a workgroup share the component and take consecutive chunks of 64 rows.
//   terms[q * K_max + k] = log_post_pred_k(row q of the list), k < K
// ---------------------------------------------------------------------------------------
#define FC_SPAN_NT 256
// The factor Lt (column j at Lt[j * D], as `pred` stores it) as the packed lower triangle the substitution reads: column j at
// Ls[j * DB - j (j - 1) / 2], entries d = j .. DB - 1, the diagonal slots holding the reciprocal pivots, zeros in the padding.
// By the whole workgroup; the caller's barrier follows.
template <int DB>
static __device__ __forceinline__ void fc_stage_tri(double *Ls, const double *Lt, int D, int tid, int nt)
{
    for (int i = tid; i < DB * DB; i += nt) {
        const int j = i / DB, d = i - j * DB;
        if (d < j) continue;
        double l = (d < D) ? Lt[j * D + d] : 0.0;           // (d >= j: d < D implies j < D)
        if (d == j) l = (j < D) ? 1. / l : 0.0;
        Ls[j * DB - j * (j - 1) / 2 + (d - j)] = l;
    }
}
// |L^-1 delta|^2 of the lane's own row, delta in registers (destroyed), the staged triangle read as same-address broadcasts:
// y_j = delta_j r_j,  s += y_j^2,  delta_d -= L_dj y_j (d > j),  j ascending.  The one copy the serial span kernel and the
// batch kernels (k_fcb_score, k_fcb_token_ll) share.
template <int DB>
static __device__ __forceinline__ double fc_subst(const double *Ls, double (&delta)[DB], int D)
{
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < DB; j++) {
        if (j < D) {                                        // (uniform)
            const double *col = Ls + (j * DB - j * (j - 1) / 2);
            const double y = delta[j] * col[0];
            s += y * y;
#pragma unroll
            for (int d = j + 1; d < DB; d++) delta[d] -= col[d - j] * y;
        }
    }
    return s;
}

template <typename XT, int DB>
__global__ __launch_bounds__(FC_SPAN_NT) void k_fc_span_terms(segk_corpus c, segk_fbgmm f, const int32_t *ids, int64_t row0, int64_t n,
                                                             double *terms)
{
    constexpr int TRI = DB * (DB + 1) / 2;
    __shared__ double Ls[TRI];                              // column j at j * DB - j (j - 1) / 2: entries d = j .. DB - 1
    __shared__ double mu[DB];
    const int k = blockIdx.y, D = c.D, tid = threadIdx.x, nt = blockDim.x;
    if (k >= *f.K) return;                                  // (workgroup-uniform)
    const double cnt = (double)f.counts[k];
    const double k_N = f.k_0 + cnt, v = f.v_0 + cnt - (double)D + 1.;
    const double *Lt = f.pred + (int64_t)k * D * D;
    fc_stage_tri<DB>(Ls, Lt, D, tid, nt);
    for (int d = tid; d < DB; d += nt) mu[d] = d < D ? f.stat_a[(int64_t)k * D + d] / k_N : 0.0;
    __syncthreads();
    const int64_t q = (int64_t)blockIdx.x * nt + tid;
    if (q >= n) return;
    const int64_t e = ids ? (int64_t)ids[q] : row0 + q;
    if (e < 0 || e >= c.n_emb) return;
    const XT *x = (const XT *)c.X + e * c.ldx;
    double delta[DB];
#pragma unroll
    for (int d = 0; d < DB; d++) delta[d] = d < D ? (double)x[d] - mu[d] : 0.0;
    const double s = fc_subst<DB>(Ls, delta, D);
    terms[q * f.K_max + k] = f.kconst[k] - 0.5 * f.log_prod[k] - (v + (double)D) / 2. * log(1. + 1. / v * s);
}

// ... then per row (a wave each): the assignment prior of fbgmm.py:268-272, the row's cached_log_prior in the slots
// k >= K, and the max-shift log-sum-exp (_cython_utils.logsumexp) into out[row].  The logits overwrite the row of `terms`.
__global__ __launch_bounds__(256) void k_fc_span_lse(segk_corpus c, segk_fbgmm f, const int32_t *ids, int64_t row0, int64_t n,
                                                     double *terms, double *out)
{
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (q >= n) return;
    const int64_t e = ids ? (int64_t)ids[q] : row0 + q;
    if (e < 0 || e >= c.n_emb) return;
    const int KM = f.K_max, K = *f.K;
    double tot = 0.0;
    for (int k = lane; k < KM; k += 64) tot += (double)f.counts[k];
    tot = fb_wave_sum(tot);                                 // exact: integer-valued
    const double lt = log(tot + f.alpha), lprior = fc_prior_rows(c, f)[e];
    double *z = terms + q * KM;
    double mx = NEG_INF_D;
    for (int k = lane; k < KM; k += 64) {
        const double zk = f.lms * (log(f.alpha / (double)KM + (double)f.counts[k]) - lt) + (k < K ? z[k] : lprior);
        z[k] = zk;                                          // (read back by the same lane below)
        mx = zk > mx ? zk : mx;
    }
    mx = fb_wave_max(mx, false);
    double s = 0.0;
    for (int k = lane; k < KM; k += 64) s += exp(z[k] - mx);
    s = fb_wave_sum(s);
    if (lane == 0) out[e] = log(s) + mx;
}

// A4: out[row] = log_marg_i(row) (fbgmm.py:256-285); one workgroup per row
template <typename XT>
__global__ __launch_bounds__(FC_NT) void k_fc_score(segk_corpus c, segk_fbgmm f, const int32_t *ids, int64_t row0, double *out)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *end;
    const FcLds S = fc_carve(smem, f.K_max, c.D, &end);
    const int64_t e = ids ? (int64_t)ids[blockIdx.x] : row0 + blockIdx.x;
    if (e < 0 || e >= c.n_emb) return;
    fc_load_row<XT>(c, e, S);
    fc_logits<XT>(c, f, e, 0, *f.K, S);
    // _cython_utils.logsumexp: max-shift, sum, log
    double mx = NEG_INF_D;
    for (int k = threadIdx.x; k < f.K_max; k += blockDim.x) mx = S.z[k] > mx ? S.z[k] : mx;
    mx = block_max(mx, S.red);
    double s = 0.0;
    for (int k = threadIdx.x; k < f.K_max; k += blockDim.x) s += exp(S.z[k] - mx);
    s = block_sum(s, S.red);
    if (threadIdx.x == 0) out[e] = log(s) + mx;
}

// out[k] = log_post_pred_k(row) for k < K, 0 for K <= k < K_max, out[K_max] = log_prior(row) evaluated from the
// prior's factor; one workgroup, a wave per component
template <typename XT>
__global__ __launch_bounds__(FC_NT) void k_fc_pred_vector(segk_corpus c, segk_fbgmm f, int64_t row, double *out)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const XT *x = (const XT *)c.X + row * c.ldx;
    const int K = *f.K;
    for (int k = w; k <= f.K_max; k += nw) {
        double v = 0.0;
        if (k < K) v = fc_post_pred<XT>(c, f, k, x, lane);
        else if (k == f.K_max) v = fc_prior_pred<XT>(c, f, x, lane);
        if (lane == 0) out[k] = v;
    }
}

// A10 for the rows new_tok[utt][0 .. n_new[utt]) in order (fbgmm.py:422-494); one workgroup
template <typename XT>
__global__ __launch_bounds__(FC_NT) void k_fc_assign(segk_corpus c, segk_fbgmm f, int utt, int map_assign, double anneal_temp,
                                                    const int32_t *new_tok, const int32_t *n_new, const double *ustream,
                                                    int64_t *ucursor, int64_t ucap, int32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *end;
    const FcLds S = fc_carve(smem, f.K_max, c.D, &end);
    int &shK = S.ctl[FC_SHK], &sh_k = S.ctl[FC_SHKNEW];
    if (threadIdx.x == 0) shK = *f.K;
    __syncthreads();
    const int nn = n_new[utt];
    for (int t = 0; t < nn; t++) {
        const int64_t e = new_tok[(int64_t)utt * c.N_max + t];
        if (e < 0 || e >= c.n_emb) continue;
        fc_load_row<XT>(c, e, S);
        const int K = shK;
        fc_logits<XT>(c, f, e, map_assign ? 2 : 1, K, S);
        fb_draw_component(f, S.z, S.red, map_assign, anneal_temp, ustream, ucursor, ucap, status, K, &sh_k);
        __syncthreads();
        const int k_new = sh_k;
        fc_add_item<XT>(c, f, e, k_new, &shK, S);
    }
    __syncthreads();
    if (threadIdx.x == 0) *f.K = shK;
}

// ---------------------------------------------------------------------------------------
// FBGMM.gibbs_sample's inner loop (fbgmm.py:352-405) over the rows ids[0 .. n) (NULL: rows 0 .. n) in order, one
// workgroup: cache the old component (statistics, factor, logdet, constant, count) in LDS, del_item with its refresh,
// logits, draw, then restore the cache (same component, no component deleted) or add_item with its refresh.
// MAP (segk_fbgmm_map_items): the MAP form of k_fbgmm_gibbs_items, described there -- fc_logits mode 2, the first maximum, no
// uniform read, *n_moved += the items that took the add_item branch without re-founding their own singleton.
// ---------------------------------------------------------------------------------------
template <typename XT, bool MAP = false>
__global__ __launch_bounds__(FC_NT) void k_fc_gibbs_items(segk_corpus c, segk_fbgmm f, const int32_t *ids, int64_t n,
                                                         int consider_unassigned, double anneal_temp, const double *ustream,
                                                         int64_t *ucursor, int64_t ucap, int32_t *status, int32_t *n_moved)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *end;
    const FcLds S = fc_carve(smem, f.K_max, c.D, &end);
    const int D = c.D, tid = threadIdx.x, nt = blockDim.x;
    const int64_t DD = (int64_t)D * D;
    double *ca = (double *)end, *cb = ca + D, *cp = cb + DD;           // [D], [D * D], [D * D]
    int &shK = S.ctl[FC_SHK], &sh_k = S.ctl[FC_SHKNEW], &sh_kold = S.ctl[FC_SHKOLD];
    int *sh_i = S.ctl + FC_SHI;
    double &sh_lp = S.dctl[0], &sh_kc = S.dctl[1];
    long long &sh_cnt = *(long long *)(S.dctl + 2);
    int moved = 0;                                           // MAP (workgroup-uniform: every term below is)
    if (tid == 0) shK = *f.K;
    __syncthreads();
    for (int64_t t = 0; t < n; t++) {
        const int64_t e = ids ? (int64_t)ids[t] : t;
        if (e < 0 || e >= c.n_emb) continue;
        __syncthreads();                                         // sh_kold / sh_k of the previous row have been read
        if (tid == 0) sh_kold = f.assignments[e];
        __syncthreads();
        const int k_old = sh_kold;
        if (!consider_unassigned && k_old == -1) continue;
        const int K_old = shK;
        const int kc = k_old < 0 ? k_old + f.K_max : k_old;      // python row -1 for an unassigned item
        for (int d = tid; d < D; d += nt) ca[d] = f.stat_a[(int64_t)kc * D + d];      // cache_component_stats
        for (int i = tid; i < D * D; i += nt) {
            cb[i] = f.stat_b[kc * DD + i];
            cp[i] = f.pred[kc * DD + i];
        }
        if (tid == 0) { sh_lp = f.log_prod[kc]; sh_kc = f.kconst[kc]; sh_cnt = f.counts[kc]; }
        fc_load_row<XT>(c, e, S);
        fc_del_item<XT>(c, f, e, &shK, sh_i, S);
        __syncthreads();
        const int K = shK;
        fc_logits<XT>(c, f, e, MAP ? 2 : 1, K, S);
        fb_draw_component(f, S.z, S.red, MAP ? 1 : 0, anneal_temp, ustream, ucursor, ucap, status, K, &sh_k);
        __syncthreads();
        const int k_new = sh_k;
        if (MAP && !(k_new == k_old && K == K_old) && !(K == K_old - 1 && k_new == K)) moved++;
        if (k_new == k_old && K == K_old) {                      // restore_component_from_stats (:397-400)
            for (int d = tid; d < D; d += nt) f.stat_a[(int64_t)kc * D + d] = ca[d];
            for (int i = tid; i < D * D; i += nt) {
                f.stat_b[kc * DD + i] = cb[i];
                f.pred[kc * DD + i] = cp[i];
            }
            if (tid == 0) {
                f.log_prod[kc] = sh_lp;
                f.kconst[kc] = sh_kc;
                f.counts[kc] = sh_cnt;
                f.assignments[e] = k_old;
            }
            __syncthreads();
        } else {
            fc_add_item<XT>(c, f, e, k_new, &shK, S);
        }
    }
    __syncthreads();
    if (tid == 0) *f.K = shK;
    if (MAP && tid == 0) *n_moved += moved;
}

// ======================================================================================
// launchers (segk_fbgmm.hip routes cov_type 2 here after its own argument checks)
// ======================================================================================
#define FC_DISPATCH_XT(c, ...)                      \
    do {                                            \
        if ((c)->x_dtype == SEGK_F32) {             \
            typedef float XT;                       \
            __VA_ARGS__                             \
        } else {                                    \
            typedef double XT;                      \
            __VA_ARGS__                             \
        }                                           \
    } while (0)

int segk_fc_check(const segk_corpus *c, const segk_fbgmm *f, const char *who)
{
    if (c->D > FC_DMAX) {
        segk_set_error("%s: full-covariance components (cov_type 2) support D <= %d, got %d", who, FC_DMAX, c->D);
        return SEGK_ERR_UNSUPPORTED;
    }
    if (f->lm_unigram) {
        segk_set_error("%s: full-covariance components (cov_type 2) take no language model", who);
        return SEGK_ERR_UNSUPPORTED;
    }
    SEGK_REQUIRE(f->prior_c != NULL, "cov_type 2: prior_c must point to D * D + n_emb + 1 doubles");
    SEGK_REQUIRE(fc_lds_bytes(f->K_max, c->D) + (size_t)(2 * c->D * c->D + c->D) * sizeof(double) <= 150 * 1024,
                 "K_max too large for the LDS logits buffer");
    return SEGK_OK;
}

int segk_fc_init_stats(segk_ctx *ctx, const segk_corpus *c, segk_fbgmm *f, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const int D = c->D;
    SEGK_CHECK_HIP(hipMemsetAsync(f->K, 0, sizeof(int32_t), st));
    SEGK_CHECK_HIP(hipMemsetAsync((void *)(f->prior_c + (int64_t)D * D + c->n_emb), 0, sizeof(double), st));
    const int32_t *blk_lo = nullptr, *sorted = nullptr, *koff = nullptr;
    int n_blocks = 0;
    int rc = segk_rows_by_label(ctx, f->assignments, c->n_emb, f->K_max, &blk_lo, &n_blocks, &sorted, &koff, stream);
    if (rc) return rc;
    const size_t lds = fc_lds_bytes(f->K_max, D);
    FC_DISPATCH_XT(c, {
        SEGK_CHECK_HIP(segk_dyn_lds((const void *)k_fc_init<XT>, lds));
        hipLaunchKernelGGL(k_fc_init<XT>, dim3((unsigned)f->K_max + 1), dim3(FC_NT), lds, st, *c, *f, blk_lo, n_blocks, sorted, koff);
        SEGK_LAUNCH_CHECK();
        if (c->n_emb > 0)
            hipLaunchKernelGGL(k_fc_prior_rows<XT>, dim3((unsigned)((c->n_emb + 3) / 4)), dim3(256), 0, st, *c, *f);
    });
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

int segk_fc_update(const segk_corpus *c, segk_fbgmm *f, int op, int utt, int64_t item, int k, const uint8_t *boundaries, void *stream)
{
    if (op == 0) {
        SEGK_REQUIRE(c->vec_ids && c->lengths && boundaries, "cov_type 2, op 0 needs the corpus's utterances and the boundaries");
        SEGK_REQUIRE(utt >= 0 && utt < c->n_utt, "utterance out of range");
        const size_t lds0 = fc_lds_bytes(f->K_max, c->D);
        FC_DISPATCH_XT(c, {
            SEGK_CHECK_HIP(segk_dyn_lds((const void *)k_fc_del_utt<XT>, lds0));
            hipLaunchKernelGGL(k_fc_del_utt<XT>, dim3(1), dim3(FC_NT), lds0, (hipStream_t)stream, *c, *f, utt, boundaries);
        });
        SEGK_LAUNCH_CHECK();
        return SEGK_OK;
    }
    SEGK_REQUIRE(op == 4 || (item >= 0 && item < c->n_emb), "item out of range");
    SEGK_REQUIRE(op == 2 || (k >= 0 && k < f->K_max), "component out of range");
    const size_t lds = fc_lds_bytes(f->K_max, c->D);
    FC_DISPATCH_XT(c, {
        SEGK_CHECK_HIP(segk_dyn_lds((const void *)k_fc_update<XT>, lds));
        hipLaunchKernelGGL(k_fc_update<XT>, dim3(1), dim3(FC_NT), lds, (hipStream_t)stream, *c, *f, op, item, k);
    });
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

// Lists of at least FC_SPAN_MIN rows go through k_fc_span_terms + k_fc_span_lse, shorter ones (log_marg_i, a few ids)
// stay on k_fc_score: two launches and a workgroup per component do not pay for a handful of rows (profiles/README.md
// "Full-covariance segmenter").  SEGK_FC_SPAN_MIN overrides the threshold (a launch-plan switch for measurements: the
// two paths sum |L^-1 delta|^2 and the logits in different orders and agree to the last bits only).
#define FC_SPAN_MIN 16

template <typename XT>
static int fc_span_launch(const segk_corpus *c, const segk_fbgmm *f, const int32_t *ids, int64_t row0, int64_t n, double *terms,
                          hipStream_t st)
{
    const int chunks = (int)((n + 63) / 64);
    const int nt = 64 * (chunks < FC_SPAN_NT / 64 ? chunks : FC_SPAN_NT / 64);
    const dim3 grid((unsigned)((n + nt - 1) / nt), (unsigned)f->K_max);
#define FC_SPAN_CASE(DB)                                                                                              \
    case DB:                                                                                                          \
        hipLaunchKernelGGL((k_fc_span_terms<XT, DB>), grid, dim3(nt), 0, st, *c, *f, ids, row0, n, terms);             \
        break;
    switch ((c->D + 7) & ~7) {
        FC_SPAN_CASE(8) FC_SPAN_CASE(16) FC_SPAN_CASE(24) FC_SPAN_CASE(32) FC_SPAN_CASE(40) FC_SPAN_CASE(48) FC_SPAN_CASE(56)
        FC_SPAN_CASE(64)
    default:
        segk_set_error("cov_type 2: no span-score kernel for D = %d", c->D);
        return SEGK_ERR_UNSUPPORTED;
    }
#undef FC_SPAN_CASE
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

int segk_fc_score(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const int32_t *ids, int64_t row0, int64_t n, double *out,
                  void *stream)
{
    SEGK_REQUIRE(ids != NULL || (row0 >= 0 && row0 + n <= c->n_emb), "rows out of range");
    if (n >= segk_env_int("SEGK_FC_SPAN_MIN", FC_SPAN_MIN) && f->K_max <= 65535) {
        SEGK_REQUIRE(ctx, "ctx");
        hipStream_t st = (hipStream_t)stream;
        // (sized for the longest utterance's triangle at once: the buffer is not replaced from one utterance to the next)
        const int64_t tri = (int64_t)c->N_max * (c->N_max + 1) / 2;
        const int64_t need = (n > tri ? n : tri) * f->K_max;
        if (int rc = segk_ws_grow(ctx, &ctx->fc_terms, &ctx->fc_terms_n, need, (size_t)need * sizeof(double), st)) return rc;
        int rc;
        FC_DISPATCH_XT(c, rc = fc_span_launch<XT>(c, f, ids, row0, n, ctx->fc_terms, st););
        if (rc) return rc;
        hipLaunchKernelGGL(k_fc_span_lse, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, *c, *f, ids, row0, n, ctx->fc_terms, out);
        SEGK_LAUNCH_CHECK();
        return SEGK_OK;
    }
    const size_t lds = fc_lds_bytes(f->K_max, c->D);
    FC_DISPATCH_XT(c, {
        SEGK_CHECK_HIP(segk_dyn_lds((const void *)k_fc_score<XT>, lds));
        hipLaunchKernelGGL(k_fc_score<XT>, dim3((unsigned)n), dim3(FC_NT), lds, (hipStream_t)stream, *c, *f, ids, row0, out);
    });
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

int segk_fc_pred_vector(const segk_corpus *c, const segk_fbgmm *f, int64_t row, double *out, void *stream)
{
    FC_DISPATCH_XT(c, hipLaunchKernelGGL(k_fc_pred_vector<XT>, dim3(1), dim3(FC_NT), 0, (hipStream_t)stream, *c, *f, row, out););
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

int segk_fc_assign(const segk_corpus *c, segk_fbgmm *f, int utt, int map_assign, double anneal_temp, const int32_t *new_tok,
                   const int32_t *n_new, const double *ustream, int64_t *ucursor, int64_t ucap, int32_t *status, void *stream)
{
    const size_t lds = fc_lds_bytes(f->K_max, c->D);
    FC_DISPATCH_XT(c, {
        SEGK_CHECK_HIP(segk_dyn_lds((const void *)k_fc_assign<XT>, lds));
        hipLaunchKernelGGL(k_fc_assign<XT>, dim3(1), dim3(FC_NT), lds, (hipStream_t)stream, *c, *f, utt, map_assign, anneal_temp,
                           new_tok, n_new, ustream, ucursor, ucap, status);
    });
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

int segk_fc_gibbs_items(const segk_corpus *c, segk_fbgmm *f, const int32_t *ids, int64_t n, int consider_unassigned,
                        double anneal_temp, const double *ustream, int64_t *ucursor, int64_t ucap, int32_t *status, void *stream,
                        int32_t *n_moved)
{
    const size_t lds = fc_lds_bytes(f->K_max, c->D) + (size_t)(2 * c->D * c->D + c->D) * sizeof(double);
    FC_DISPATCH_XT(c, {
        if (n_moved) {                                       // the MAP sweep of segk_fbgmm_map_items
            SEGK_CHECK_HIP(segk_dyn_lds((const void *)k_fc_gibbs_items<XT, true>, lds));
            hipLaunchKernelGGL((k_fc_gibbs_items<XT, true>), dim3(1), dim3(FC_NT), lds, (hipStream_t)stream, *c, *f, ids, n,
                               consider_unassigned, anneal_temp, ustream, ucursor, ucap, status, n_moved);
        } else {
            SEGK_CHECK_HIP(segk_dyn_lds((const void *)k_fc_gibbs_items<XT>, lds));
            hipLaunchKernelGGL(k_fc_gibbs_items<XT>, dim3(1), dim3(FC_NT), lds, (hipStream_t)stream, *c, *f, ids, n,
                               consider_unassigned, anneal_temp, ustream, ucursor, ucap, status, n_moved);
        }
    });
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

// ======================================================================================
// Batch sampler (segk_fbbatch.hip, specification tests/fullcov_batch.py on oracle/np_fbgmm_batch.py): the cov_type 2 forms
// of the kernels of one Gibbs step.  State is the batch's own (segk_fbatch, cov_type 2 shapes): nothing here writes the serial view
// (stat_a / stat_b / pred / log_prod / kconst / K), which segk_fbgmm_init_stats rebuilds when the batch state is materialised.
//   k_fcb_partials    counts, sum x and the packed triangle of sum outer(x, x) of a (block, slice) cell: a workgroup per
//                     (slice, slot), a thread per triangle entry, the slot's tokens (k_fbb_sort's list) walked in order
//   k_fcb_prepare     a workgroup per slot: every entry of the record summed without block b in the specification's order,
//                     covar formed in LDS and factored, the slot's tables written
//   k_fcb_score       span scores of the block's rows: a workgroup of 256 rows (a lane per row) walks the occupied slots,
//                     staging each factor's triangle in LDS, an online log-sum-exp per lane -- no (rows x K_max) buffer
//   k_fcb_token_ll    token likelihoods of the block's new segments into a table of the context, same substitution body
// ======================================================================================
template <typename XT>
__global__ __launch_bounds__(FC_NT) void k_fcb_partials(segk_corpus c, segk_fbgmm f, segk_fbatch bt, int s_lo, int b,
                                                       const int32_t *sorted, int64_t sorted_stride, const int32_t *koff)
{
    const int tid = threadIdx.x, nt = blockDim.x, D = c.D, KM = f.K_max;
    // (the step's totals are cleared here, as by the other types' kernels: see k_fbb_partials)
    if (blockIdx.x == 0 && tid < 2) bt.scal[tid] = 0.0;
    const int si = blockIdx.x / KM, s = s_lo + si, k = blockIdx.x - si * KM;
    const int32_t *list = sorted + (int64_t)si * sorted_stride;
    const int q0 = koff[(int64_t)si * (KM + 1) + k], q1 = koff[(int64_t)si * (KM + 1) + k + 1];
    const XT *X = (const XT *)c.X;
    // every thread owns the entries tid, tid + nt, ... of the D x D square that lie in the lower triangle and, below D, one
    // of sum x; the tokens are walked in order by all of them (k_fc_init)
    constexpr int PER = FC_DMAX * FC_DMAX / FC_NT;
    double acc[PER], am = 0.0;
    int ia[PER], ib[PER];
    bool own[PER];
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int i = tid + q * nt;
        acc[q] = 0.0;
        ib[q] = i / D;                                      // column
        ia[q] = i - ib[q] * D;                              // row
        own[q] = i < D * D && ia[q] >= ib[q];
        if (!own[q]) ia[q] = ib[q] = 0;
    }
    for (int t = q0; t < q1; t++) {
        const int64_t e = list[t];
        if (e < 0 || e >= c.n_emb) continue;                // (uniform)
        const XT *x = X + e * c.ldx;
#pragma unroll
        for (int r = 0; r < PER; r++)
            if (own[r]) acc[r] += fc_xprod<XT>(x[ia[r]], x[ib[r]]);
        if (tid < D) am += (double)x[tid];
    }
    double *rec = bt.partials + ((int64_t)b * bt.n_slices + s) * fbb_rec(f, D);
    if (tid == 0) rec[k] = (double)(q1 - q0);
    if (tid < D) rec[KM + (int64_t)k * D + tid] = am;
    double *tri = rec + KM + (int64_t)KM * D + (int64_t)k * fbb_tri(D);
#pragma unroll
    for (int q = 0; q < PER; q++)
        if (own[q]) tri[fbb_tri_index(D, ia[q], ib[q])] = acc[q];
}

#define FCB_PREP_NT 256
static size_t fcb_prepare_lds(int D) { return (size_t)(16 * FCB_PREP_NT + D * D + 3 * D + 16 + 2) * sizeof(double); }

__global__ __launch_bounds__(FCB_PREP_NT) void k_fcb_prepare(segk_corpus c, segk_fbgmm f, segk_fbatch bt, int b, double prior_alpha)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, nt = blockDim.x, D = c.D, KM = f.K_max, k = blockIdx.x, S = bt.n_slices;
    double *scr = (double *)smem;                           // [16 slices][nt]
    double *A = scr + 16 * FCB_PREP_NT;                     // [D * D] column j contiguous
    double *diag = A + D * D;                               // [D]
    double *mN = diag + D;                                  // [D]
    double *sxs = mN + D;                                   // [D]
    double *red = sxs + D;                                  // [16]
    double *shn = red + 16;                                 // [1]
    const int64_t rec = fbb_rec(f, D);
    const int T = fbb_tri(D);
    double *my = scr + tid;
    // every entry of the slot's record without block b: blocks ascending inside a slice, the slices by the tree
    if (tid == 0) {
        fbb_sum_slices(bt, rec, k, b, my, FCB_PREP_NT);
        shn[0] = fbb_tree(my, S, FCB_PREP_NT);
    } else if (tid >= 64 && tid < 64 + D) {
        const int d = tid - 64;
        fbb_sum_slices(bt, rec, KM + (int64_t)k * D + d, b, my, FCB_PREP_NT);
        sxs[d] = fbb_tree(my, S, FCB_PREP_NT);
    }
    const int64_t tri0 = KM + (int64_t)KM * D + (int64_t)k * T;
    for (int i = tid; i < D * D; i += nt) {
        const int j = i / D, d = i - j * D;
        if (d < j) continue;
        fbb_sum_slices(bt, rec, tri0 + fbb_tri_index(D, d, j), b, my, FCB_PREP_NT);
        const double sxx = fbb_tree(my, S, FCB_PREP_NT);
        // S = (S_0 + k_0 m_0 m_0') + sxx: the prior term first (add_item of a new component, then the tokens)
        A[i] = (f.prior_a[d * D + j] + f.k_0 * (f.prior_b[d] * f.prior_b[j])) + sxx;
    }
    __syncthreads();
    const double n = shn[0];
    const double k_N = f.k_0 + n, v_N = f.v_0 + n, v = v_N - (double)D + 1.;
    if (tid < D) mN[tid] = (f.k_0 * f.prior_b[tid] + sxs[tid]) / k_N;
    __syncthreads();
    double lconst = 0.0;
    if (n > 0.0) {                                          // (uniform)
        const double scale = (k_N + 1.) / (k_N * (v_N - (double)D + 1.));
        for (int i = tid; i < D * D; i += nt) {
            const int j = i / D, d = i - j * D;
            if (d >= j) A[i] = scale * (A[i] - k_N * (mN[d] * mN[j]));
        }
        const bool ok = fc_cholesky(A, diag, D);
        if (!ok) {
            // (no previous factor to keep in batch mode: the sweep's status check raises)
            if (tid == 0) atomicOr(fc_status(c, f), FC_STATUS_PIVOT);
        } else {
            double *pp = bt.q_t + (int64_t)k * D * D;
            for (int i = tid; i < D * D; i += nt) {
                const int j = i / D, d = i - j * D;
                pp[i] = d > j ? A[i] : (d == j ? diag[j] : 0.0);
            }
            const double tot = block_sum(tid < D ? log(diag[tid]) : 0.0, red);
            lconst = fc_const(D, v) - 0.5 * (2. * tot);
        }
    }
    if (tid < D) bt.mean_t[(int64_t)k * D + tid] = mN[tid];
    if (tid == 0) {
        bt.cnt[k] = n;
        bt.lconst[k] = lconst;
        bt.zconst[k] = f.lms * log(prior_alpha / (double)KM + n) + (n > 0.0 ? lconst : 0.0);
        bt.half[k] = (v + (double)D) / 2.;
        atomicAdd(&bt.scal[0], n);                          // integer valued: exact in any order
        if (n > 0.0) atomicAdd(&bt.scal[1], 1.0);
    }
}

#define FCB_NT 256
#define FCB_KMAX 1024                  // slots of the batch form (the occupancy flags of k_fcb_score, k_fbb_sort's one thread per slot)
template <typename XT, int DB>
__global__ __launch_bounds__(FCB_NT) void k_fcb_score(segk_corpus c, segk_fbgmm f, segk_fbatch bt, FbbMap map, int b, double prior_alpha,
                                                     double *score)
{
    constexpr int TRI = DB * (DB + 1) / 2;
    __shared__ double Ls[TRI];
    __shared__ double mu[DB];
    __shared__ uint8_t occ[FCB_KMAX];
    const int D = c.D, KM = f.K_max, tid = threadIdx.x, nt = blockDim.x;
    int s, idx;
    if (!fbb_locate(map, blockIdx.x, &s, &idx)) return;     // (workgroup-uniform)
    const int slice = map.lo[s];
    const int64_t r_lo = bt.row_range[(slice * bt.n_blocks + b) * 2], r_hi = bt.row_range[(slice * bt.n_blocks + b) * 2 + 1];
    const int64_t row = r_lo + (int64_t)idx * FCB_NT + tid;
    const bool valid = row < r_hi && row >= 0 && row < c.n_emb;
    const XT *x = (const XT *)c.X + (valid ? row : 0) * c.ldx;
    for (int k = tid; k < KM; k += nt) occ[k] = bt.cnt[k] > 0.0;
    double mx = NEG_INF_D, sm = 0.0;
    for (int k = 0; k < KM; k++) {
        __syncthreads();                                    // the flags are written; the previous slot's triangle has been read
        if (!occ[k]) continue;                              // (uniform)
        fc_stage_tri<DB>(Ls, bt.q_t + (int64_t)k * D * D, D, tid, nt);
        for (int d = tid; d < DB; d += nt) mu[d] = d < D ? bt.mean_t[(int64_t)k * D + d] : 0.0;
        __syncthreads();
        if (valid) {
            double delta[DB];
#pragma unroll
            for (int d = 0; d < DB; d++) delta[d] = d < D ? (double)x[d] - mu[d] : 0.0;
            const double sq = fc_subst<DB>(Ls, delta, D);
            const double v = f.v_0 + bt.cnt[k] - (double)D + 1.;
            const double z = bt.zconst[k] - bt.half[k] * log(1. + 1. / v * sq);
            if (z > mx) {
                sm = sm * exp(mx - z) + 1.0;                // exp(-inf) = 0 on the first value
                mx = z;
            } else {
                sm += exp(z - mx);
            }
        }
    }
    if (!valid) return;
    // the empty slots share one value: lms log(alpha / K_max) + the row's prior predictive
    const double n_empty = (double)KM - bt.scal[1];
    if (n_empty > 0.0) {
        const double z = f.lms * log(prior_alpha / (double)KM) + bt.prior_rows[row];
        if (z > mx) {
            sm = sm * exp(mx - z) + n_empty;
            mx = z;
        } else {
            sm += n_empty * exp(z - mx);
        }
    }
    score[row] = log(sm) + mx - f.lms * log(bt.scal[0] + prior_alpha);
}

template <typename XT, int DB>
__global__ __launch_bounds__(FCB_NT) void k_fcb_token_ll(segk_corpus c, segk_fbgmm f, segk_fbatch bt, int s_lo, int b,
                                                        const int32_t *new_tok, const int32_t *n_new, double *ll, int u_cap)
{
    constexpr int TRI = DB * (DB + 1) / 2;
    __shared__ double Ls[TRI];
    __shared__ double mu[DB];
    const int D = c.D, KM = f.K_max, NM = c.N_max, tid = threadIdx.x, nt = blockDim.x;
    const int k = blockIdx.y, si = blockIdx.z, slice = s_lo + si;
    const int u0 = bt.utt_range[(slice * bt.n_blocks + b) * 2], u1 = bt.utt_range[(slice * bt.n_blocks + b) * 2 + 1];
    if ((int64_t)blockIdx.x * nt >= (int64_t)(u1 - u0) * NM) return;     // (workgroup-uniform)
    const bool occupied = bt.cnt[k] > 0.0;                  // (uniform)
    if (occupied) {
        fc_stage_tri<DB>(Ls, bt.q_t + (int64_t)k * D * D, D, tid, nt);
        for (int d = tid; d < DB; d += nt) mu[d] = d < D ? bt.mean_t[(int64_t)k * D + d] : 0.0;
    }
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * nt + tid;
    const int ui = (int)(p / NM), t = (int)(p - (int64_t)ui * NM);
    const int utt = u0 + ui;
    if (utt >= u1 || ui >= u_cap || t >= n_new[utt]) return;
    const int64_t e = new_tok[(int64_t)utt * NM + t];
    if (e < 0 || e >= c.n_emb) return;
    const int64_t r = ((int64_t)si * u_cap + ui) * NM + t;  // (< local slices * u_cap * N_max rows: the launcher's allocation)
    double v = bt.prior_rows[e];
    if (occupied) {
        const XT *x = (const XT *)c.X + e * c.ldx;
        double delta[DB];
#pragma unroll
        for (int d = 0; d < DB; d++) delta[d] = d < D ? (double)x[d] - mu[d] : 0.0;
        const double sq = fc_subst<DB>(Ls, delta, D);
        const double dof = f.v_0 + bt.cnt[k] - (double)D + 1.;
        v = bt.lconst[k] - bt.half[k] * log(1. + 1. / dof * sq);
    }
    ll[r * KM + k] = v;
}

int segk_fcb_check(const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, const char *who)
{
    if (c->D > FC_DMAX) {
        segk_set_error("%s: full-covariance components (cov_type 2) support D <= %d, got %d", who, FC_DMAX, c->D);
        return SEGK_ERR_UNSUPPORTED;
    }
    if (f->lm_unigram) {
        segk_set_error("%s: full-covariance components (cov_type 2) take no language model", who);
        return SEGK_ERR_UNSUPPORTED;
    }
    if (f->K_max > FCB_KMAX) {
        segk_set_error("%s: the batch sampler takes full-covariance components (cov_type 2) with K_max <= %d, got %d", who, FCB_KMAX,
                       f->K_max);
        return SEGK_ERR_UNSUPPORTED;
    }
    SEGK_REQUIRE(f->prior_c != NULL, "cov_type 2: prior_c must point to D * D + n_emb + 1 doubles");
    SEGK_REQUIRE(bt->mean_t && bt->q_t && bt->prior_rows, "cov_type 2: mean_t [K_max, D] / q_t [K_max, D, D] / prior_rows missing");
    return SEGK_OK;
}

int segk_fcb_partials(const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, int s_lo, int s_n, int b,
                      const int32_t *sorted, int64_t sorted_stride, const int32_t *koff, void *stream)
{
    FC_DISPATCH_XT(c, hipLaunchKernelGGL(k_fcb_partials<XT>, dim3((unsigned)(s_n * f->K_max)), dim3(FC_NT), 0, (hipStream_t)stream, *c, *f,
                                          *bt, s_lo, b, sorted, sorted_stride, koff););
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

int segk_fcb_prepare(const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, int b, void *stream)
{
    const size_t lds = fcb_prepare_lds(c->D);
    SEGK_CHECK_HIP(segk_dyn_lds((const void *)k_fcb_prepare, lds));
    hipLaunchKernelGGL(k_fcb_prepare, dim3((unsigned)f->K_max), dim3(FCB_PREP_NT), lds, (hipStream_t)stream, *c, *f, *bt, b, f->alpha);
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

#define FCB_DB_SWITCH(D, CASE)                                                                        \
    switch (((D) + 7) & ~7) {                                                                         \
        CASE(8) CASE(16) CASE(24) CASE(32) CASE(40) CASE(48) CASE(56) CASE(64)                        \
    default:                                                                                          \
        segk_set_error("cov_type 2: no batch kernel for D = %d", (D));                                \
        return SEGK_ERR_UNSUPPORTED;                                                                  \
    }

template <typename XT>
static int fcb_score_launch(const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, const FbbMap &m, int n_wg, int b,
                            double *score, hipStream_t st)
{
#define FCB_CASE(DB)                                                                                                              \
    case DB:                                                                                                                      \
        hipLaunchKernelGGL((k_fcb_score<XT, DB>), dim3((unsigned)n_wg), dim3(FCB_NT), 0, st, *c, *f, *bt, m, b, f->alpha, score);   \
        break;
    FCB_DB_SWITCH(c->D, FCB_CASE)
#undef FCB_CASE
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

int segk_fcb_score(const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, int s_lo, int s_n, int b, const int32_t *n_rows,
                   double *score, void *stream)
{
    SEGK_REQUIRE(s_n >= 1 && s_n <= 16, "at most 16 local slices");
    // (256 rows per workgroup at every block size: a wave of 64 rows per workgroup, tried for blocks that leave compute units
    // idle, was slower -- profiles/README.md "Full-covariance batch sampler")
    const int nt = FCB_NT;
    FbbMap m;
    m.n = s_n;
    m.off[0] = 0;
    for (int s = 0; s < s_n; s++) {
        m.lo[s] = s_lo + s;
        m.off[s + 1] = m.off[s] + (n_rows[s] + nt - 1) / nt;
    }
    if (m.off[s_n] == 0) return SEGK_OK;
    int rc;
    FC_DISPATCH_XT(c, rc = fcb_score_launch<XT>(c, f, bt, m, m.off[s_n], b, score, (hipStream_t)stream););
    return rc;
}

template <typename XT>
static int fcb_token_launch(const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, dim3 grid, int s_lo, int b,
                            const int32_t *new_tok, const int32_t *n_new, double *ll, int u_cap, hipStream_t st)
{
#define FCB_CASE(DB)                                                                                                              \
    case DB:                                                                                                                      \
        hipLaunchKernelGGL((k_fcb_token_ll<XT, DB>), grid, dim3(FCB_NT), 0, st, *c, *f, *bt, s_lo, b, new_tok, n_new, ll, u_cap);  \
        break;
    FCB_DB_SWITCH(c->D, FCB_CASE)
#undef FCB_CASE
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

int segk_fcb_token_ll(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, int s_lo, int s_n, int b,
                      const int32_t *n_utts, const int32_t *new_tok, const int32_t *n_new, const double **ll, int *u_cap,
                      void *stream)
{
    SEGK_REQUIRE(ctx, "context");
    int u_most = 0;
    for (int s = 0; s < s_n; s++) u_most = n_utts[s] > u_most ? n_utts[s] : u_most;
    *u_cap = u_most;
    *ll = nullptr;
    if (u_most == 0) return SEGK_OK;
    // (bounded by the token positions of one block of the local slices)
    const int64_t need = (int64_t)s_n * u_most * c->N_max * f->K_max;
    if (int rc = segk_ws_grow(ctx, &ctx->fcb_ll, &ctx->fcb_ll_n, need, (size_t)need * sizeof(double), (hipStream_t)stream)) return rc;
    *ll = ctx->fcb_ll;
    const dim3 grid((unsigned)(((int64_t)u_most * c->N_max + FCB_NT - 1) / FCB_NT), (unsigned)f->K_max, (unsigned)s_n);
    int rc;
    FC_DISPATCH_XT(c, rc = fcb_token_launch<XT>(c, f, bt, grid, s_lo, b, new_tok, n_new, ctx->fcb_ll, u_most, (hipStream_t)stream););
    return rc;
}

int segk_fc_prior_rows_view(const segk_corpus *c, const segk_fbgmm *f, double *out, void *stream)
{
    SEGK_REQUIRE(c && f && out && f->prior_c && c->D <= FC_DMAX, "cov_type 2: the prior's factor in prior_c, D <= 64");
    if (c->n_emb == 0) return SEGK_OK;
    FC_DISPATCH_XT(c, hipLaunchKernelGGL(k_fc_prior_rows_view<XT>, dim3((unsigned)((c->n_emb + 3) / 4)), dim3(256), 0,
                                          (hipStream_t)stream, *c, *f, out););
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}
