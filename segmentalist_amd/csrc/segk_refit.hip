// segk_refit.hip -- batch refit of the k-means statistics between two batch sweeps (specification:
// tests/kmeans_refit.py kmeans_batch_refit).  A Lloyd iteration over the current tokens in the batch mode's own terms: the
// token rows are scored (segk_kmeans_score / segk_kmeans_score_hinted on the id list made here), their labels rewritten in the
// slot arrays, and segk_kmeans_batch_partials / segk_kmeans_batch_finalize rebuild the statistics from them as after a sweep.
// Plain grids of independent workgroups; atomics on integers only: every result is independent of the execution order.
#include "segk_kmeans_dev.h"

#define REFIT_CHUNK 1024            /* slots per workgroup of the two collection kernels (4 per thread) */

// live slots (k >= 0, as k_batch_sort_sum reads them) of every chunk of REFIT_CHUNK slots behind p0
__global__ __launch_bounds__(256) void k_refit_count(const int32_t *new_k, int64_t p0, int64_t S, int32_t *chunk_cnt)
{
    __shared__ int32_t wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * REFIT_CHUNK;
    int n = 0;
#pragma unroll
    for (int q = 0; q < REFIT_CHUNK / 256; q++) {
        const int64_t s = base + q * 256 + tid;
        n += (s < S && new_k[p0 + s] >= 0) ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if (lane == 0) wsum[wv] = n;
    __syncthreads();
    if (tid == 0) chunk_cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// the rows of the live slots as a dense list in slot order: a workgroup places its chunk's behind the chunks in front of it
// (their counts from k_refit_count); entries [count, n_list) are -1, which the score calls skip
__global__ __launch_bounds__(256) void k_refit_collect(const int32_t *new_tok, const int32_t *new_k, int64_t p0, int64_t S,
                                                       const int32_t *chunk_cnt, int n_chunks, int32_t *ids, int32_t *slots,
                                                       int64_t n_list, int32_t *count_out, int32_t *status)
{
    __shared__ int32_t red[2][4], wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c = blockIdx.x;
    int before = 0, total = 0;
    for (int i = tid; i < n_chunks; i += 256) {
        const int v = chunk_cnt[i];
        total += v;
        if (i < c) before += v;
    }
    for (int o = 32; o > 0; o >>= 1) {
        before += __shfl_xor(before, o);
        total += __shfl_xor(total, o);
    }
    if (lane == 0) { red[0][wv] = before; red[1][wv] = total; }
    __syncthreads();
    before = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    total = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    const int64_t base = (int64_t)c * REFIT_CHUNK;
    int64_t pos = before;
    for (int q = 0; q < REFIT_CHUNK / 256; q++) {
        const int64_t s = base + q * 256 + tid;
        const bool live = s < S && new_k[p0 + s] >= 0;
        const unsigned long long bal = __ballot(live);
        __syncthreads();                                   // (the previous round's counts have been read)
        if (lane == 0) wcnt[wv] = __popcll(bal);
        __syncthreads();
        int off = __popcll(bal & ((1ull << lane) - 1ull));
        for (int w = 0; w < wv; w++) off += wcnt[w];
        if (live && pos + off < n_list) {
            ids[pos + off] = new_tok[p0 + s];
            if (slots) slots[pos + off] = (int32_t)(p0 + s);
        }
        pos += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    }
    // the list's tail: S >= n_list, so the chunks cover it
    for (int i = tid; i < REFIT_CHUNK; i += 256) {
        const int64_t p = (int64_t)total + base + i;
        if (p < n_list) {
            ids[p] = -1;
            if (slots) slots[p] = -1;
        }
    }
    if (c == 0 && tid == 0) {
        *count_out = total;
        if (total > n_list) atomicOr(status, 8);
    }
}

// new_k[slot] = cand.k[row] for the live slots of utterances [lo, hi), one wave per utterance: n_flag as k_kmeans_segment
// leaves it (tokens naming an inactive row), the changed labels counted into *moved
__global__ __launch_bounds__(256) void k_refit_apply(const int32_t *cand_k, int64_t n_emb, const int32_t *new_tok, int32_t *new_k,
                                                     int lo, int hi, int N_max, const int32_t *K_dev, int32_t *n_flag,
                                                     int32_t *moved, int32_t *status)
{
    const int lane = threadIdx.x & 63;
    const int u = lo + (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (u >= hi) return;
    const int Kact = *K_dev;
    int nf = 0, nm = 0, bad = 0;
    for (int j = lane; j < N_max; j += 64) {
        const int64_t p = (int64_t)u * N_max + j;
        const int k_old = new_k[p];
        if (k_old < 0) continue;
        const int64_t e = new_tok[p];
        const int k = (e >= 0 && e < n_emb) ? cand_k[e] : -1;
        if (k < 0) { bad = 1; continue; }                  // (a token the score call did not reach: the label stays)
        nf += k >= Kact ? 1 : 0;
        nm += k != k_old ? 1 : 0;
        new_k[p] = k;
    }
    for (int o = 32; o > 0; o >>= 1) {
        nf += __shfl_xor(nf, o);
        nm += __shfl_xor(nm, o);
        bad |= __shfl_xor(bad, o);
    }
    if (lane == 0) {
        n_flag[u] = nf;
        if (nm) atomicAdd(moved, nm);
        if (bad) atomicOr(status, 8);
    }
}

// cand.k of every row through a relabel table: the label a hint stands for after clean_components, -1 (no hint) for
// anything outside [0, K_max) before or after the translation -- what K1's label map makes of hint and table per launch
__global__ __launch_bounds__(256) void k_hint_relabel(int32_t *cand_k, int64_t n, const int32_t *table, int K_max)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int k = cand_k[e];
    int v = (k >= 0 && k < K_max) ? table[k] : -1;
    if (v < 0 || v >= K_max) v = -1;
    if (v != k) cand_k[e] = v;
}

__global__ void k_refit_put_moved(double *out, const int32_t *moved) { out[7] = (double)*moved; }

extern "C" {

int64_t segk_kmeans_refit_scratch_words(int64_t n_slots) { return n_slots > 0 ? (n_slots + REFIT_CHUNK - 1) / REFIT_CHUNK : 1; }

int32_t segk_kmeans_refit_collect(segk_ctx *ctx, const segk_corpus *c, int32_t utt_lo, int32_t utt_hi, const int32_t *new_tok,
                                  const int32_t *new_k, int32_t *chunk_scratch, int32_t *ids, int32_t *slots, int64_t n_list,
                                  int32_t *count_out, int32_t *status, void *stream)
{
    (void)ctx;
    int rc = check_corpus(c);
    if (rc) return rc;
    SEGK_REQUIRE(new_tok && new_k && chunk_scratch && ids && count_out && status, "refit_collect operands");
    SEGK_REQUIRE(c->n_utt > 0 && c->N_max > 0, "corpus without utterances");
    SEGK_REQUIRE(0 <= utt_lo && utt_lo <= utt_hi && utt_hi <= c->n_utt, "utterance range");
    SEGK_REQUIRE((int64_t)c->n_utt * c->N_max < ((int64_t)1 << 31), "token slots are int32");
    const int64_t S = (int64_t)(utt_hi - utt_lo) * c->N_max, p0 = (int64_t)utt_lo * c->N_max;
    SEGK_REQUIRE(n_list >= 0 && n_list <= S && n_list <= c->n_emb, "0 <= n_list <= min(slots of the range, n_emb)");
    hipStream_t st = (hipStream_t)stream;
    if (S == 0) {
        SEGK_CHECK_HIP(hipMemsetAsync(count_out, 0, sizeof(int32_t), st));
        return SEGK_OK;
    }
    const int n_chunks = (int)((S + REFIT_CHUNK - 1) / REFIT_CHUNK);
    hipLaunchKernelGGL(k_refit_count, dim3(n_chunks), dim3(256), 0, st, new_k, p0, S, chunk_scratch);
    hipLaunchKernelGGL(k_refit_collect, dim3(n_chunks), dim3(256), 0, st, new_tok, new_k, p0, S, chunk_scratch, n_chunks, ids, slots,
                       n_list, count_out, status);
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

int32_t segk_kmeans_refit_apply(segk_ctx *ctx, const segk_corpus *c, const segk_kmeans *m, const segk_cand *cand, int32_t utt_lo,
                                int32_t utt_hi, const int32_t *new_tok, int32_t *new_k, int32_t *n_flag, int32_t *moved,
                                int32_t *status, void *stream)
{
    int rc = check_corpus(c);
    if (rc) return rc;
    SEGK_REQUIRE(m && m->K && cand && cand->k && new_tok && new_k && n_flag && moved && status, "refit_apply operands");
    SEGK_REQUIRE(c->n_utt > 0 && c->N_max > 0, "corpus without utterances");
    SEGK_REQUIRE(0 <= utt_lo && utt_lo <= utt_hi && utt_hi <= c->n_utt, "utterance range");
    // the labels under the next finalize change behind the delta pass's back: its state is not carried across a refit
    if (ctx) {
        ctx->delta_valid = 0;
        segk_delta_pending_drop(ctx);
    }
    hipStream_t st = (hipStream_t)stream;
    SEGK_CHECK_HIP(hipMemsetAsync(moved, 0, sizeof(int32_t), st));
    if (utt_hi == utt_lo) return SEGK_OK;
    hipLaunchKernelGGL(k_refit_apply, dim3((unsigned)((utt_hi - utt_lo + 3) / 4)), dim3(256), 0, st, cand->k, c->n_emb, new_tok, new_k,
                       utt_lo, utt_hi, c->N_max, m->K, n_flag, moved, status);
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

int32_t segk_kmeans_hint_relabel(segk_ctx *ctx, const segk_corpus *c, const segk_kmeans *m, const segk_cand *cand,
                                 const int32_t *table, void *stream)
{
    (void)ctx;
    int rc = check_corpus(c);
    if (rc) return rc;
    SEGK_REQUIRE(m && m->K_max >= 1 && cand && cand->k && table, "hint_relabel operands");
    hipLaunchKernelGGL(k_hint_relabel, dim3((unsigned)((c->n_emb + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cand->k, c->n_emb,
                       table, m->K_max);
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

int32_t segk_kmeans_refit_record(segk_ctx *ctx, const segk_corpus *c, const segk_kmeans *m, int32_t utt_lo, int32_t utt_hi,
                                 const int32_t *new_tok, const int32_t *new_k, const int32_t *status, const int32_t *moved,
                                 double *out_scalars, void *stream)
{
    SEGK_REQUIRE(moved, "refit_record operands");
    int rc = segk_kmeans_batch_record(ctx, c, m, utt_lo, utt_hi, new_tok, new_k, status, out_scalars, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_refit_put_moved, dim3(1), dim3(1), 0, (hipStream_t)stream, out_scalars, moved);
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

}  // extern "C"
