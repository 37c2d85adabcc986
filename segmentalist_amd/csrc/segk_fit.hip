// segk_fit.hip -- one Lloyd iteration of KMeans.fit (kmeans.py:97-173) on the device, with the reference's bits (DESIGN.md 4.19;
// specification: tests/kmeans_fit_device.py).  Every decision is taken against the means frozen at the start of the iteration,
// so the iteration is: score the items -> the moved items as a dense list in item order -> add_item's clamp replayed over the
// moves that name an inactive row -> the 2 * moved del/add operations bucketed by component, in order -> one workgroup per
// component walks its operations with dev_del_item's / dev_add_item's float64 arithmetic (segk_stats.hip:128-184) -> the labels
// -> clean_components -> the operand images -> the record.  Plain grids of independent workgroups; atomics on integers only
// (histogram, status bits); every placement is computed, none depends on the execution order.
#include "segk_kmeans_dev.h"

#define FIT_CHUNK 1024              /* items per workgroup of the collection kernels (4 per thread) */
#define FIT_OPS 512                 /* operations per workgroup of the histogram and placement kernels (2 per thread) */
#define FIT_BATCH 16                /* rows k_fit_apply fetches ahead of the additions */
#define FIT_KMAX 8192               /* the histogram's LDS: K_max counters */

// ctl words: [0] moves listed, [1] of them naming a row >= K, [2] items, [3] K at the start, [4] moves found
#define FIT_CTL 8

struct FitScratch {
    int32_t *ctl, *ids, *cnt_a, *cnt_b, *mv_row, *mv_old, *mv_fin, *hi_idx, *hi_req, *tot, *comp_off, *sorted, *relog, *hist;
    int64_t n_row_chunks, n_item_chunks, n_op_chunks, words;
};

static FitScratch fit_carve(int32_t *base, int64_t n_emb, int64_t n_max, int K_max)
{
    FitScratch s;
    s.n_row_chunks = (n_emb + FIT_CHUNK - 1) / FIT_CHUNK;
    s.n_item_chunks = (n_max + FIT_CHUNK - 1) / FIT_CHUNK;
    s.n_op_chunks = (2 * n_max + FIT_OPS - 1) / FIT_OPS;
    const int64_t nc = s.n_row_chunks > s.n_item_chunks ? s.n_row_chunks : s.n_item_chunks;
    int64_t o = 0;
    auto take = [&](int64_t n) { int32_t *p = base ? base + o : nullptr; o += (n + 3) & ~(int64_t)3; return p; };
    s.ctl = take(FIT_CTL);
    s.ids = take(n_max);
    s.cnt_a = take(nc);
    s.cnt_b = take(nc);
    s.mv_row = take(n_max);
    s.mv_old = take(n_max);
    s.mv_fin = take(n_max);
    s.hi_idx = take(n_max);
    s.hi_req = take(n_max);
    s.tot = take(K_max);
    s.comp_off = take((int64_t)K_max + 1);
    s.sorted = take(2 * n_max);
    s.relog = take(1 + 2 * (int64_t)K_max);
    s.hist = take(s.n_op_chunks * K_max);
    s.words = o;
    return s;
}

// sum of v[0..c) and of v[0..n) by the whole workgroup of 256 threads
__device__ __forceinline__ void fit_prefix(const int32_t *v, int n, int c, int32_t (*red)[4], int &before, int &total)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int b = 0, t = 0;
    for (int i = tid; i < n; i += 256) {
        const int x = v[i];
        t += x;
        if (i < c) b += x;
    }
    for (int o = 32; o > 0; o >>= 1) {
        b += __shfl_xor(b, o);
        t += __shfl_xor(t, o);
    }
    __syncthreads();                                       // (an earlier use of `red` has been read)
    if (lane == 0) { red[0][wv] = b; red[1][wv] = t; }
    __syncthreads();
    before = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    total = red[1][0] + red[1][1] + red[1][2] + red[1][3];
}

// a flagged thread's position among the flagged threads of the workgroup, in thread order; n_out: how many there are
__device__ __forceinline__ int fit_rank(bool flag, int32_t *wcnt, int &n_out)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag);
    __syncthreads();                                       // (the previous round's counts have been read)
    if (lane == 0) wcnt[wv] = __popcll(bal);
    __syncthreads();
    int off = __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wv; w++) off += wcnt[w];
    n_out = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    return off;
}

// (1) items of consider_unassigned=False: the rows with a label, ascending (kmeans.py:118-121 skips the others)
__global__ __launch_bounds__(256) void k_fit_count_items(const int32_t *assignments, int64_t n_emb, int32_t *cnt)
{
    __shared__ int32_t wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * FIT_CHUNK;
    int n = 0;
#pragma unroll
    for (int q = 0; q < FIT_CHUNK / 256; q++) {
        const int64_t e = base + q * 256 + tid;
        n += (e < n_emb && assignments[e] != -1) ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if (lane == 0) wsum[wv] = n;
    __syncthreads();
    if (tid == 0) cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// ... as a dense list: a workgroup places its chunk's rows behind those of the chunks in front of it; entries [count, n_list)
// are -1, which the score call and k_fit_moves skip
__global__ __launch_bounds__(256) void k_fit_collect_items(const int32_t *assignments, int64_t n_emb, const int32_t *cnt, int n_chunks,
                                                           int32_t *ids, int64_t n_list, int32_t *ctl, int32_t *status)
{
    __shared__ int32_t red[2][4], wcnt[4];
    const int tid = threadIdx.x, c = blockIdx.x;
    int before, total;
    fit_prefix(cnt, n_chunks, c, red, before, total);
    const int64_t base = (int64_t)c * FIT_CHUNK;
    int64_t pos = before;
    for (int q = 0; q < FIT_CHUNK / 256; q++) {
        const int64_t e = base + q * 256 + tid;
        const bool live = e < n_emb && assignments[e] != -1;
        int n;
        const int off = fit_rank(live, wcnt, n);
        if (live && pos + off < n_list) ids[pos + off] = (int32_t)e;
        pos += n;
    }
    for (int i = tid; i < FIT_CHUNK; i += 256) {           // the list's tail: the chunks cover it (n_list <= n_emb)
        const int64_t p = (int64_t)total + base + i;
        if (p < n_list) ids[p] = -1;
    }
    if (c == 0 && tid == 0) {
        ctl[2] = total;
        if (total > n_list) atomicOr(status, 8);
    }
}

// item i of the list: its row, the label it has and the one it asks for (np.argmax of neg_sqrd_norm, left in cand.k by the score
// call) -> is it a move (kmeans.py:123-131)?  bad: a label outside what the arrays behind it hold -- never listed
__device__ __forceinline__ bool fit_item(const int32_t *ids, int64_t i, int64_t n, int64_t n_emb, const int32_t *assignments,
                                         const int32_t *cand_k, int K_max, int &row, int &k_old, int &k_req, bool &bad)
{
    bad = false;
    if (i >= n) return false;
    const int64_t e = ids ? (int64_t)ids[i] : i;
    if (e < 0) return false;
    if (e >= n_emb) { bad = true; return false; }
    row = (int)e;
    k_old = assignments[e];
    k_req = cand_k[e];
    if (k_req < 0 || k_req >= K_max || k_old < -1 || k_old >= K_max) { bad = true; return false; }
    return k_req != k_old;
}

// (3) the moves per chunk of items, and those of them that name a row >= K (add_item's clamp can only touch these)
__global__ __launch_bounds__(256) void k_fit_count_moves(const int32_t *ids, int64_t n, int64_t n_emb, const int32_t *assignments,
                                                         const int32_t *cand_k, int K_max, const int32_t *K_dev, int32_t *cnt_mv,
                                                         int32_t *cnt_hi, int32_t *status)
{
    __shared__ int32_t wsum[3][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * FIT_CHUNK;
    const int K0 = *K_dev;
    int nm = 0, nh = 0, nb = 0;
#pragma unroll
    for (int q = 0; q < FIT_CHUNK / 256; q++) {
        int row, k_old, k_req;
        bool bad;
        const bool mv = fit_item(ids, base + q * 256 + tid, n, n_emb, assignments, cand_k, K_max, row, k_old, k_req, bad);
        nm += mv ? 1 : 0;
        nh += (mv && k_req >= K0) ? 1 : 0;
        nb += bad ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) {
        nm += __shfl_xor(nm, o);
        nh += __shfl_xor(nh, o);
        nb += __shfl_xor(nb, o);
    }
    if (lane == 0) { wsum[0][wv] = nm; wsum[1][wv] = nh; wsum[2][wv] = nb; }
    __syncthreads();
    if (tid == 0) {
        cnt_mv[blockIdx.x] = wsum[0][0] + wsum[0][1] + wsum[0][2] + wsum[0][3];
        cnt_hi[blockIdx.x] = wsum[1][0] + wsum[1][1] + wsum[1][2] + wsum[1][3];
        if (wsum[2][0] + wsum[2][1] + wsum[2][2] + wsum[2][3]) atomicOr(status, 8);
    }
}

// ... as dense lists in item order: move j = (mv_row, mv_old, mv_fin = the requested label until k_fit_clamp has run); the
// moves naming a row >= K again as (hi_idx = j, hi_req).  cap: entries each list holds
__global__ __launch_bounds__(256) void k_fit_moves(const int32_t *ids, int64_t n, int64_t n_emb, const int32_t *assignments,
                                                   const int32_t *cand_k, int K_max, const int32_t *K_dev, const int32_t *cnt_mv,
                                                   const int32_t *cnt_hi, int n_chunks, int64_t cap, int range_items, int32_t *mv_row,
                                                   int32_t *mv_old, int32_t *mv_fin, int32_t *hi_idx, int32_t *hi_req, int32_t *ctl,
                                                   int32_t *status)
{
    __shared__ int32_t red[2][4], wcnt[4];
    const int tid = threadIdx.x, c = blockIdx.x;
    const int K0 = *K_dev;
    int before_m, total_m, before_h, total_h;
    fit_prefix(cnt_mv, n_chunks, c, red, before_m, total_m);
    fit_prefix(cnt_hi, n_chunks, c, red, before_h, total_h);
    const int64_t base = (int64_t)c * FIT_CHUNK;
    int64_t pm = before_m, ph = before_h;
    for (int q = 0; q < FIT_CHUNK / 256; q++) {
        int row = 0, k_old = 0, k_req = 0;
        bool bad;
        const bool mv = fit_item(ids, base + q * 256 + tid, n, n_emb, assignments, cand_k, K_max, row, k_old, k_req, bad);
        const bool hi = mv && k_req >= K0;
        int nm, nh;
        const int om = fit_rank(mv, wcnt, nm);
        const int oh = fit_rank(hi, wcnt, nh);
        if (mv && pm + om < cap) {
            mv_row[pm + om] = row;
            mv_old[pm + om] = k_old;
            mv_fin[pm + om] = k_req;
            if (hi && ph + oh < cap) {
                hi_idx[ph + oh] = (int32_t)(pm + om);
                hi_req[ph + oh] = k_req;
            }
        }
        pm += nm;
        ph += nh;
    }
    if (c == 0 && tid == 0) {
        ctl[0] = total_m < cap ? total_m : (int32_t)cap;
        ctl[1] = total_m <= cap ? total_h : 0;             // (lists that do not hold every move are not used: status bit 8)
        if (range_items >= 0) ctl[2] = range_items;
        ctl[3] = K0;
        ctl[4] = total_m;
        if (total_m > cap) atomicOr(status, 8);
    }
}

// (4) add_item's clamp (kmeans_components.py:101-104: k > K -> K, k == K -> K += 1) replayed over the moves naming a row >= K,
// in item order, by one wave: 64 of them per round, and per round one ballot for every component founded in it -- the first
// lane still asking for a row >= K founds component K, the lanes in front of it keep what they asked for.  At most K_max - K
// foundings; once K == K_max nothing can be clamped any more.
__global__ __launch_bounds__(64) void k_fit_clamp(const int32_t *ctl, const int32_t *hi_idx, const int32_t *hi_req, int32_t *mv_fin,
                                                  int32_t *K_dev, int K_max)
{
    const int lane = threadIdx.x;
    const int H = ctl[1];
    int K = ctl[3];
    for (int h0 = 0; h0 < H && K < K_max; h0 += 256) {
        int req[4], idx[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {                      // four rounds' loads in flight together
            const int h = h0 + q * 64 + lane;
            req[q] = h < H ? hi_req[h] : -1;
            idx[q] = h < H ? hi_idx[h] : -1;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            int fin = req[q];
            unsigned long long pending = ~0ull;
            for (;;) {
                const unsigned long long mask = __ballot(req[q] >= K) & pending;
                if (!mask) break;
                const int f = __ffsll((long long)mask) - 1;
                if (lane == f) fin = K;
                K++;
                pending = f == 63 ? 0ull : (~0ull << (f + 1));
            }
            if (idx[q] >= 0 && fin != req[q]) mv_fin[idx[q]] = fin;
        }
    }
    if (lane == 0) *K_dev = K;
}

// operation o of the iteration: o = 2j the delete of move j (none for an item without a label), o = 2j + 1 its add
__device__ __forceinline__ int fit_op_key(const int32_t *mv_old, const int32_t *mv_fin, int o)
{
    return (o & 1) ? mv_fin[o >> 1] : mv_old[o >> 1];
}

// (5) the operations per component and chunk of FIT_OPS operations
__global__ __launch_bounds__(256) void k_fit_hist(const int32_t *ctl, const int32_t *mv_old, const int32_t *mv_fin, int K_max,
                                                  int32_t *hist)
{
    extern __shared__ int32_t h_lds[];
    const int tid = threadIdx.x;
    const int n_ops = 2 * ctl[0];
    const int base = (int)blockIdx.x * FIT_OPS;
    if (base >= n_ops) return;
    for (int k = tid; k < K_max; k += 256) h_lds[k] = 0;
    __syncthreads();
    for (int i = tid; i < FIT_OPS; i += 256) {
        const int o = base + i;
        if (o < n_ops) {
            const int key = fit_op_key(mv_old, mv_fin, o);
            if (key >= 0 && key < K_max) atomicAdd(&h_lds[key], 1);
        }
    }
    __syncthreads();
    for (int k = tid; k < K_max; k += 256) hist[(int64_t)blockIdx.x * K_max + k] = h_lds[k];
}

// ... per component: the chunk counts into the chunk's offset inside the component's list, and the component's total
__global__ __launch_bounds__(256) void k_fit_scan_chunks(const int32_t *ctl, int K_max, int32_t *hist, int32_t *tot)
{
    const int k = (int)blockIdx.x * 256 + threadIdx.x;
    if (k >= K_max) return;
    const int nc = (2 * ctl[0] + FIT_OPS - 1) / FIT_OPS;
    int run = 0;
    for (int c = 0; c < nc; c++) {
        const int v = hist[(int64_t)c * K_max + k];
        hist[(int64_t)c * K_max + k] = run;
        run += v;
    }
    tot[k] = run;
}

// ... and the components' lists one behind the other: comp_off[k] = sum of tot[0..k), comp_off[K_max] = the operations listed
__global__ __launch_bounds__(256) void k_fit_scan_comp(const int32_t *tot, int K_max, int32_t *comp_off)
{
    __shared__ int32_t seg[256];
    const int tid = threadIdx.x;
    const int per = (K_max + 255) / 256;
    const int lo = tid * per < K_max ? tid * per : K_max, hi = lo + per < K_max ? lo + per : K_max;
    int s = 0;
    for (int k = lo; k < hi; k++) s += tot[k];
    seg[tid] = s;
    __syncthreads();
    int run = 0;
    for (int t = 0; t < tid; t++) run += seg[t];
    for (int k = lo; k < hi; k++) {
        comp_off[k] = run;
        run += tot[k];
    }
    if (tid == 255) comp_off[K_max] = run;
}

// ... every operation to its place: behind the component's operations of the chunks in front, then behind those of its own
// chunk with a smaller number (counted, not taken from an atomic: the order inside a component is the operations' own).
// sorted: the row of an add, ~row of a delete
__global__ __launch_bounds__(256) void k_fit_place(const int32_t *ctl, const int32_t *mv_row, const int32_t *mv_old, const int32_t *mv_fin,
                                                   int K_max, const int32_t *hist, const int32_t *comp_off, int64_t cap_ops,
                                                   int32_t *sorted)
{
    __shared__ int32_t keys[FIT_OPS];
    const int tid = threadIdx.x;
    const int n_ops = 2 * ctl[0];
    const int base = (int)blockIdx.x * FIT_OPS;
    if (base >= n_ops) return;
    for (int i = tid; i < FIT_OPS; i += 256) {
        const int o = base + i;
        int key = -1;
        if (o < n_ops) {
            key = fit_op_key(mv_old, mv_fin, o);
            if (key >= K_max) key = -1;
        }
        keys[i] = key;
    }
    __syncthreads();
    for (int i = tid; i < FIT_OPS; i += 256) {
        const int key = keys[i];
        if (key < 0) continue;
        int rank = 0;
        for (int j = 0; j < i; j++) rank += keys[j] == key ? 1 : 0;
        const int o = base + i;
        const int64_t pos = (int64_t)comp_off[key] + hist[(int64_t)blockIdx.x * K_max + key] + rank;
        const int row = mv_row[o >> 1];
        if (pos < cap_ops) sorted[pos] = (o & 1) ? row : ~row;
    }
}

// (6) one workgroup per component with operations, thread d owns dimension d (and d + blockDim ...): the component's deletes and
// adds strictly in order, numerator -= / += X[i] in float64 and the count alongside, exactly dev_del_item / dev_add_item
// (segk_stats.hip:128-184; kmeans_components.py:106-110, 124-131).  The rows do not depend on the additions: they are fetched
// FIT_BATCH at a time, the next batch in flight while the additions of the current one run; only the additions are sequential.
// means[k] is written once, from the last operation that left the count non-zero (the reference rewrites it after every such
// operation; DESIGN.md 4.19 on why no one can tell).
template <typename XT>
__device__ __forceinline__ void fit_fetch(const XT *__restrict__ X, int64_t ldx, int d, const int32_t *__restrict__ sorted, int p, int hi,
                                          int32_t (&code)[FIT_BATCH], XT (&x)[FIT_BATCH])
{
#pragma unroll
    for (int b = 0; b < FIT_BATCH; b++) code[b] = p + b < hi ? sorted[p + b] : 0;
#pragma unroll
    for (int b = 0; b < FIT_BATCH; b++) {
        const int64_t row = code[b] < 0 ? (int64_t)~code[b] : (int64_t)code[b];
        x[b] = p + b < hi ? X[row * ldx + d] : (XT)0;
    }
}

template <typename XT>
__device__ __forceinline__ void fit_walk(const int32_t (&code)[FIT_BATCH], const XT (&x)[FIT_BATCH], int p, int hi, double &v, int64_t &cnt,
                                         double &last_v, int64_t &last_c)
{
#pragma unroll
    for (int b = 0; b < FIT_BATCH; b++) {
        if (p + b < hi) {
            if (code[b] < 0) {
                v = v - (double)x[b];
                cnt -= 1;
            } else {
                v = v + (double)x[b];
                cnt += 1;
            }
            if (cnt != 0) {
                last_v = v;
                last_c = cnt;
            }
        }
    }
}

template <typename XT>
__global__ __launch_bounds__(256) void k_fit_apply(segk_corpus c, segk_kmeans m, const int32_t *__restrict__ comp_off,
                                                   const int32_t *__restrict__ sorted)
{
    const int k = blockIdx.x;
    const int lo = comp_off[k], hi = comp_off[k + 1];
    if (lo == hi) return;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int D = c.D;
    const XT *X = (const XT *)c.X;
    XT *means = (XT *)m.means;
    const int64_t cnt0 = m.counts[k];
    int64_t cnt_end = cnt0;
    for (int d = tid; d < D; d += nt) {
        double v = m.mean_numerators[(int64_t)k * D + d];
        int64_t cnt = cnt0, last_c = 0;
        double last_v = 0.0;
        int32_t ca[FIT_BATCH], cb[FIT_BATCH];
        XT xa[FIT_BATCH], xb[FIT_BATCH];
        fit_fetch<XT>(X, c.ldx, d, sorted, lo, hi, ca, xa);
        for (int p = lo; p < hi; p += 2 * FIT_BATCH) {
            fit_fetch<XT>(X, c.ldx, d, sorted, p + FIT_BATCH, hi, cb, xb);
            fit_walk<XT>(ca, xa, p, hi, v, cnt, last_v, last_c);
            fit_fetch<XT>(X, c.ldx, d, sorted, p + 2 * FIT_BATCH, hi, ca, xa);
            fit_walk<XT>(cb, xb, p + FIT_BATCH, hi, v, cnt, last_v, last_c);
        }
        m.mean_numerators[(int64_t)k * D + d] = v;
        if (last_c != 0) means[(int64_t)k * D + d] = (XT)(last_v / (double)last_c);
        cnt_end = cnt;
    }
    __syncthreads();                                       // (every thread has read counts[k])
    if (tid == 0) m.counts[k] = cnt_end;
}

// ... and the moved items' labels (add_item's assignments[i] = k, kmeans_components.py:111)
__global__ __launch_bounds__(256) void k_fit_assign(const int32_t *ctl, const int32_t *mv_row, const int32_t *mv_fin, int32_t *assignments)
{
    const int j = (int)blockIdx.x * 256 + threadIdx.x;
    if (j < ctl[0]) assignments[mv_row[j]] = mv_fin[j];
}

// (8) the record (kmeans.py:150-153) beside sum_neg_sqrd_norm, which segk_kmeans_sum_neg_sqrd_norm has put into record[4]
__global__ void k_fit_record(const int32_t *ctl, const int32_t *K_dev, const int32_t *status, double *record)
{
    record[0] = (double)ctl[4];
    record[1] = (double)*K_dev;
    record[2] = (double)ctl[2];
    record[3] = (double)ctl[3];
    record[5] = (double)status[0];
    record[6] = (double)status[1];
    record[7] = (double)ctl[1];
}

extern "C" {

int64_t segk_kmeans_fit_scratch_words(int64_t n_emb, int64_t n_items_max, int32_t K_max)
{
    if (n_emb < 1 || n_items_max < 1 || K_max < 1) return 0;
    return fit_carve(nullptr, n_emb, n_items_max, K_max).words;
}

int32_t segk_kmeans_fit_step(segk_ctx *ctx, const segk_corpus *c, segk_kmeans *m, const segk_cand *cand, int32_t consider_unassigned,
                             int64_t n_items_max, int32_t *scratch, double *record, int32_t *status, void *stream)
{
    SEGK_REQUIRE(ctx, "ctx");
    int rc = check_corpus(c);
    if (rc) return rc;
    SEGK_REQUIRE(m && m->means && m->mean_numerators && m->counts && m->random_means && m->assignments && m->K && cand && cand->k &&
                 scratch && record && status, "fit_step operands");
    SEGK_REQUIRE(m->K_max >= 1 && m->K_max <= FIT_KMAX, "fit_step supports K_max <= 8192");
    SEGK_REQUIRE(c->n_emb < ((int64_t)1 << 31), "rows are int32");
    SEGK_REQUIRE(n_items_max >= 1 && n_items_max <= c->n_emb && n_items_max < ((int64_t)1 << 29), "1 <= n_items_max <= n_emb");
    SEGK_REQUIRE(!consider_unassigned || n_items_max == c->n_emb, "consider_unassigned: every row is an item (n_items_max == n_emb)");
    hipStream_t st = (hipStream_t)stream;
    const FitScratch s = fit_carve(scratch, c->n_emb, n_items_max, m->K_max);
    // the labels and the means change behind the delta score pass's back, as under add_item / del_item: its state is not
    // carried across a fit (the score call below drops it as well, unless it has no rows)
    ctx->delta_valid = 0;
    segk_delta_pending_drop(ctx);
    // (1) the items, (2) their np.argmax into cand->k
    const int32_t *ids = nullptr;
    if (!consider_unassigned) {
        hipLaunchKernelGGL(k_fit_count_items, dim3((unsigned)s.n_row_chunks), dim3(256), 0, st, m->assignments, c->n_emb, s.cnt_a);
        hipLaunchKernelGGL(k_fit_collect_items, dim3((unsigned)s.n_row_chunks), dim3(256), 0, st, m->assignments, c->n_emb, s.cnt_a,
                           (int)s.n_row_chunks, s.ids, n_items_max, s.ctl, status);
        SEGK_LAUNCH_CHECK();
        ids = s.ids;
    }
    rc = segk_kmeans_score(ctx, c, m, ids, 0, n_items_max, cand, status, stream);
    if (rc) return rc;
    // (3) the moves, (4) their final labels and the new K
    const int nic = (int)s.n_item_chunks;
    hipLaunchKernelGGL(k_fit_count_moves, dim3((unsigned)nic), dim3(256), 0, st, ids, n_items_max, c->n_emb, m->assignments, cand->k,
                       m->K_max, m->K, s.cnt_a, s.cnt_b, status);
    hipLaunchKernelGGL(k_fit_moves, dim3((unsigned)nic), dim3(256), 0, st, ids, n_items_max, c->n_emb, m->assignments, cand->k, m->K_max,
                       m->K, s.cnt_a, s.cnt_b, nic, n_items_max, consider_unassigned ? (int)c->n_emb : -1, s.mv_row, s.mv_old, s.mv_fin,
                       s.hi_idx, s.hi_req, s.ctl, status);
    hipLaunchKernelGGL(k_fit_clamp, dim3(1), dim3(64), 0, st, s.ctl, s.hi_idx, s.hi_req, s.mv_fin, m->K, m->K_max);
    // (5) the operations by component, in order
    const size_t lds = (size_t)m->K_max * sizeof(int32_t);
    hipLaunchKernelGGL(k_fit_hist, dim3((unsigned)s.n_op_chunks), dim3(256), lds, st, s.ctl, s.mv_old, s.mv_fin, m->K_max, s.hist);
    hipLaunchKernelGGL(k_fit_scan_chunks, dim3((unsigned)((m->K_max + 255) / 256)), dim3(256), 0, st, s.ctl, m->K_max, s.hist, s.tot);
    hipLaunchKernelGGL(k_fit_scan_comp, dim3(1), dim3(256), 0, st, s.tot, m->K_max, s.comp_off);
    hipLaunchKernelGGL(k_fit_place, dim3((unsigned)s.n_op_chunks), dim3(256), 0, st, s.ctl, s.mv_row, s.mv_old, s.mv_fin, m->K_max, s.hist,
                       s.comp_off, 2 * n_items_max, s.sorted);
    // (6) the statistics and the labels
    const int nt = c->D <= 64 ? 64 : c->D <= 128 ? 128 : 256;
    DISPATCH_XT(c, hipLaunchKernelGGL(k_fit_apply<XT>, dim3((unsigned)m->K_max), dim3(nt), 0, st, *c, *m, s.comp_off, s.sorted););
    hipLaunchKernelGGL(k_fit_assign, dim3((unsigned)((n_items_max + 255) / 256)), dim3(256), 0, st, s.ctl, s.mv_row, s.mv_fin,
                       m->assignments);
    SEGK_LAUNCH_CHECK();
    // (7) clean_components (kmeans_components.py:263-266) and the filters' operand images
    rc = segk_launch_clean(c, m, status, st, s.relog);
    if (rc) return rc;
    rc = segk_kmeans_prepare(ctx, c, m, stream);
    if (rc) return rc;
    // (8) the record
    rc = segk_kmeans_sum_neg_sqrd_norm(ctx, c, m, record + 4, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_fit_record, dim3(1), dim3(1), 0, st, s.ctl, m->K, status, record);
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

}  // extern "C"
