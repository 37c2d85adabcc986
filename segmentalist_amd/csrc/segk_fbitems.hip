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
//                           k_fbb_slots forms for the same row and statistics.  The tile's logits [64][K_max] stay in LDS
//                           where they fit (FBI_LDS_MAX) and go to a workspace of the context otherwise; then one wave per
//                           item: prior term, softmax, annealing and draw (fbb_draw_row, the call k_fbb_slots makes).
//   cov_type 2              the likelihoods of the block's items are formed by k_fcb_token_ll (segk_fullcov.hip: one slot's
//                           packed triangle staged per 256 items) into its context table; k_fbi_assign<XT, 2> is the draw half
//                           reading that table.
//   k_fbi_assign_diag32<XT> cov_type 1 with the Student-t terms in float32 on the hardware logarithm (segk_fbi_assign_diag32;
//                           described where it stands): rows and slot tables staged as float32, the draw half unchanged.
//
// The same tile serves the TOKEN step of the unigram segmenter's acoustic-model batch sweep (segk_fbt_assign: the inner sweeps
// of UnigramAcousticWordseg.gibbs_sample(..., am_n_iter, am_sync="batch"); specification tests/am_batch.py): the boundaries are
// frozen, every current token of block b is resampled against the statistics of all other blocks.
//
//   k_fbt_compact           one workgroup per local slice: an ordered scan of n_new over the cell's utterances writes the cell's
//                           token list (row, utterance, position) and its length into a workspace of the context -- utterance
//                           order, then position, the order of the partial sums
//   k_fbi_assign<.., true>  a tile is 64 consecutive entries of that list (TOK): the rows are gathered through it, the draw of
//                           token t of utterance i uses u01(seed, sweep, i, N_max + t) as k_fbb_slots does, n_new / new_tok
//                           are only read.  The grid is sized from the host's bound on the cell's tokens (its landmarks); a
//                           tile that begins at or beyond the list's length returns at once.
//   k_fbi_assign_diag32<.., true>  the same axis on the float32 form (segk_fbt_assign_diag32: the inner sweeps of
//                           am_sweep(..., score_precision="f32"), diagonal components; tests/am_batch_f32.py)
// And it serves the ORPHAN pass of FBGMM.set_K(..., sync="batch") (segk_fbi_assign_orphans; fbgmm.py:174-180 as one blocked
// pass; specification tests/fbgmm_set_k.py): the items that lost their component when the bank was cut to its K largest are
// few and scattered, so they are listed like tokens.
//
//   k_fbi_orphans           one workgroup per local slice: an ordered scan over the cell's items writes the ids of its orphans
//                           (was[i] >= 0, slot[i] < 0), in index order, into the token lists' workspace as (row i, utterance i,
//                           position 0) and marks n_new[i] = 1 -- the item holds a slot once the tile kernel has run
//   k_fbi_assign<.., true>  as for tokens: with N_max = 1 the draw of entry (i, 0) uses u01(seed, sweep, i, 1), the uniform of
//                           k_fbi_assign<.., false> for item i, and with cov_type 2 its row of k_fcb_token_ll's table is item
//                           i's.  Always the fp64 likelihoods (bt.mean_t / q_t), also on a sweeper of float32 scores.
// And it serves the MAP sweeps of FBGMM.map_assign(sync="batch") (segk_fbi_assign_map / _map_diag32; fbgmm.py:465-494 on slots;
// specification tests/fbgmm_items_map.py): the MAP template axis of k_fbi_assign and of the float32 tile body
// (k_fbi_assign_map_diag32 beside k_fbi_assign_diag32), items only.  The likelihood half and
// probe_ll as they stand; the draw half (prior term with lms, softmax, annealing, inverse-CDF walk) becomes fbb_map_row
// (segk_fbb_dev.h, the body of k_fbb_slots<.., MAP>) on pz[k] = log(alpha / K_max + n_k), staged once per workgroup as a 65th
// row of the tile's logits, and the items whose slot changed are counted.
// No grid barrier, no spin loop, no cooperative launch: a plain grid over the tiles.  One atomic, in the MAP half only: a
// workgroup's count of moved items is added to the caller's counter with one integer atomicAdd (the sum does not depend on the
// order of the workgroups or of the launches of a block); the sampled forms use none.
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

// the token lists of block b of the local slices (k_fbt_compact writes, k_fbi_assign<.., true> reads): local slice s owns the
// entries off[s] .. off[s + 1] - 1 (the host's bound on its tokens), the first count[s] of them are tokens
struct FbtList {
    int32_t *count;             // [16]
    int32_t *row, *utt, *pos;   // [off[n]] each
    int off[17];
};

#define FBT_NT 256
__global__ __launch_bounds__(FBT_NT) void k_fbt_compact(segk_corpus c, segk_fbatch bt, FbtList L, int s_lo, int b, const int32_t *new_tok,
                                                       const int32_t *n_new)
{
    __shared__ int sc[FBT_NT];
    const int s = blockIdx.x, slice = s_lo + s, tid = threadIdx.x, NM = c.N_max;
    const int u0 = bt.utt_range[(slice * bt.n_blocks + b) * 2], u1 = bt.utt_range[(slice * bt.n_blocks + b) * 2 + 1];
    const int o0 = L.off[s], cap = L.off[s + 1] - o0;
    int base = 0;                                           // tokens of the utterances before this pass (uniform)
    for (int c0 = u0; c0 < u1; c0 += FBT_NT) {
        const int utt = c0 + tid;
        int n = utt < u1 ? n_new[utt] : 0;
        n = n < 0 ? 0 : (n > NM ? NM : n);
        sc[tid] = n;
        __syncthreads();
        for (int o = 1; o < FBT_NT; o <<= 1) {              // inclusive scan, utterance order
            const int v = tid >= o ? sc[tid - o] : 0;
            __syncthreads();
            sc[tid] += v;
            __syncthreads();
        }
        const int first = base + sc[tid] - n;
        for (int t = 0; t < n; t++) {
            const int j = first + t;
            if (j >= cap) break;                            // (never: cap counts the cell's landmarks)
            L.row[o0 + j] = new_tok[(int64_t)utt * NM + t];
            L.utt[o0 + j] = utt;
            L.pos[o0 + j] = t;
        }
        base += sc[FBT_NT - 1];
        __syncthreads();
    }
    if (tid == 0) L.count[s] = base < cap ? base : cap;
}

// The orphans of block b of the local slices, listed for k_fbi_assign<.., true>: item i of the cell with was[i] >= 0 (it held a
// component before FBGMM.set_K cut the bank) and bt.slot[i] < 0 (its component went).  k_fbt_compact's scan with one entry per
// orphan: row = utterance = i, position 0.  n_new[i] = 1 is written here: the tile kernel gives every listed item a slot, and with
// cov_type 2 k_fcb_token_ll evaluates the items n_new names.
__global__ __launch_bounds__(FBT_NT) void k_fbi_orphans(segk_corpus c, segk_fbatch bt, FbtList L, int s_lo, int b, const int32_t *was,
                                                       int32_t *n_new)
{
    __shared__ int sc[FBT_NT];
    const int s = blockIdx.x, slice = s_lo + s, tid = threadIdx.x;
    const int u0 = bt.utt_range[(slice * bt.n_blocks + b) * 2], u1 = bt.utt_range[(slice * bt.n_blocks + b) * 2 + 1];
    const int o0 = L.off[s], cap = L.off[s + 1] - o0;
    int base = 0;                                           // orphans among the items before this pass (uniform)
    for (int c0 = u0; c0 < u1; c0 += FBT_NT) {
        const int i = c0 + tid;
        const int n = i < u1 && i >= 0 && i < c.n_emb && was[i] >= 0 && bt.slot[i] < 0 ? 1 : 0;
        sc[tid] = n;
        __syncthreads();
        for (int o = 1; o < FBT_NT; o <<= 1) {              // inclusive scan, index order
            const int v = tid >= o ? sc[tid - o] : 0;
            __syncthreads();
            sc[tid] += v;
            __syncthreads();
        }
        const int j = base + sc[tid] - n;
        if (n && j < cap) {                                 // (always: cap counts the cell's items)
            L.row[o0 + j] = i;
            L.utt[o0 + j] = i;
            L.pos[o0 + j] = 0;
            n_new[i] = 1;
        }
        base += sc[FBT_NT - 1];
        __syncthreads();
    }
    if (tid == 0) L.count[s] = base < cap ? base : cap;
}

// n_new[i] = 1 for every item of block b of the local slices (consider_unassigned with cov_type 2: k_fcb_token_ll evaluates the
// tokens n_new names)
__global__ __launch_bounds__(256) void k_fbi_mark(segk_fbatch bt, int s_lo, int b, int32_t *n_new)
{
    const int slice = s_lo + blockIdx.y;
    const int u0 = bt.utt_range[(slice * bt.n_blocks + b) * 2], u1 = bt.utt_range[(slice * bt.n_blocks + b) * 2 + 1];
    const int i = u0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (i < u1) n_new[i] = 1;
}

// The MAP half of the item kernels' draw loops (MAP = true), one wave: the slot of item i by fbb_map_row on the staged prior
// terms, written like a draw; returns 1 where the item's slot changed (an unassigned item that gets one counts).
static __device__ __forceinline__ int fbi_map_item(const segk_fbatch &bt, const double *pz, const double *zr, int KM, int i,
                                                   int32_t *n_new, int lane)
{
    const int old = bt.slot[i];                             // (wave-uniform)
    const int k = fbb_map_row(pz, zr, KM, lane);
    if (lane == 0) {
        bt.slot[i] = k;
        n_new[i] = 1;
    }
    return k != old ? 1 : 0;
}

// ... and its end: the waves' counts of moved items summed in LDS, ONE integer add per workgroup to *n_moved (an integer sum:
// the result does not depend on the order in which the workgroups, or the launches of a block, arrive)
static __device__ __forceinline__ void fbi_map_count(int moved, int w, int nw, int lane, int32_t *n_moved)
{
    __shared__ int sh_moved[16];                            // (nw <= 16: the waves of the larger of the two kernels)
    if (lane == 0) sh_moved[w] = moved;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int j = 0; j < nw; j++) tot += sh_moved[j];
        if (tot) atomicAdd(n_moved, tot);
    }
}

// TOK = false: the items of the stand-alone model; TOK = true: the tokens of a segmenter's cell through the lists `L`
// MAP (items only; segk_fbi_assign_map, specification tests/fbgmm_items_map.py): the draw half replaced by the hard assignment
// of FBGMM.map_assign_i (fbgmm.py:465-494) on slots -- pz[k] = log(alpha / K_max + n_k) (no lms: fbgmm.py:475-479) staged once
// per workgroup as a 65th row of the tile's logits (LDS or the workspace, wherever they are; with cov_type 2 the K_max doubles
// are the kernel's whole LDS), then per item one wave: fbb_map_row, the slot written, the items whose slot changed counted into
// *n_moved.  No temperature, no uniform, no softmax: `sweep` and `anneal_temp` are not read.
template <typename XT, int COV, bool TOK = false, bool MAP = false>
__global__ __launch_bounds__(FBI_NT) void k_fbi_assign(segk_corpus c, segk_fbgmm f, segk_fbatch bt, FbbMap map, int wg0, int b,
                                                      uint64_t sweep, double prior_alpha, double anneal_temp, int consider_unassigned,
                                                      int32_t *n_new, double *zbuf, const double *fc_ll, int fc_ucap,
                                                      double *probe_ll, int64_t probe_ld, FbtList L, int32_t *n_moved)
{
    static_assert(!(TOK && MAP), "the MAP half exists for items");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int D = c.D, KM = f.K_max, tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);        // (wave-uniform, and known to be)
    int s, idx;
    if (!fbb_locate(map, wg0 + blockIdx.x, &s, &idx)) return;
    const int slice = map.lo[s];
    const int u0 = bt.utt_range[(slice * bt.n_blocks + b) * 2], u1 = bt.utt_range[(slice * bt.n_blocks + b) * 2 + 1];
    int i0, nr;
    const int32_t *trow = nullptr, *tutt = nullptr, *tpos = nullptr;    // TOK: the tile's entries of the token lists
    if constexpr (TOK) {
        const int n_tok = L.count[s];
        i0 = idx * FBI_T;                                   // the tile's first token of the cell's list
        if (i0 >= n_tok) return;                            // (workgroup-uniform: the grid is sized from the host's bound)
        nr = n_tok - i0 < FBI_T ? n_tok - i0 : FBI_T;
        trow = L.row + L.off[s] + i0;
        tutt = L.utt + L.off[s] + i0;
        tpos = L.pos + L.off[s] + i0;
    } else {
        i0 = u0 + idx * FBI_T;                              // the tile's first item
        nr = u1 - i0 < FBI_T ? u1 - i0 : FBI_T;             // (>= 1: the host counts the tiles from the same ranges)
    }
    // the embedding row of the tile's entry r (TOK: -1 where the list names none -- such an entry is left alone)
    auto row_of = [&](int r) -> int64_t {
        if constexpr (TOK) {
            const int64_t e = trow[r];
            return e >= 0 && e < c.n_emb ? e : -1;
        } else
            return i0 + r;
    };
    double *ll = nullptr;                                   // [FBI_T][K_max] likelihood part of the logits, then the probabilities
    // ... of entry r
    auto row_ll = [&](int r) -> double * {
        if constexpr (TOK && COV == 2)
            // k_fcb_token_ll's table: row (local slice * u_cap + utterance of the cell) * N_max + position
            return const_cast<double *>(fc_ll) + (((int64_t)s * fc_ucap + (tutt[r] - u0)) * c.N_max + tpos[r]) * KM;
        else
            return ll + (int64_t)r * KM;
    };
    double *pz = nullptr;                                   // MAP: [K_max] log(alpha / K_max + n_k)
    if constexpr (COV == 2) {
        // k_fcb_token_ll's table: row (local slice * u_cap + item of the cell), the row's prior predictive in the empty slots
        if constexpr (!TOK) ll = const_cast<double *>(fc_ll) + ((int64_t)s * fc_ucap + (int64_t)idx * FBI_T) * KM;
        if constexpr (MAP) {
            pz = (double *)smem;
            for (int k = tid; k < KM; k += FBI_NT) pz[k] = log(prior_alpha / (double)KM + bt.cnt[k]);       // fbgmm.py:475-479
            __syncthreads();
        }
    } else {
        double *xs = (double *)smem;                        // [D][FBI_T]: the lanes' rows side by side
        double *pm = xs + (size_t)FBI_T * D;                // [FBI_KC][D][2]: (mean, q) of the staged slots
        ll = zbuf ? zbuf + (int64_t)blockIdx.x * (FBI_T + (MAP ? 1 : 0)) * KM : pm + 2 * (size_t)FBI_KC * D;
        if constexpr (MAP) {                                // (published by the barriers of the likelihood loop)
            pz = ll + (int64_t)FBI_T * KM;
            for (int k = tid; k < KM; k += FBI_NT) pz[k] = log(prior_alpha / (double)KM + bt.cnt[k]);       // fbgmm.py:475-479
        }
        const XT *X = (const XT *)c.X;
        for (int j = tid; j < FBI_T * D; j += FBI_NT) {
            const int r = j / D, d = j - r * D;
            const int64_t e = r < nr ? row_of(r) : -1;
            xs[d * FBI_T + r] = e >= 0 ? (double)X[e * c.ldx + d] : 0.0;
        }
        const int64_t e_lane = lane < nr ? row_of(lane) : -1;
        const bool valid = e_lane >= 0;
        const double lp = valid ? bt.prior_rows[e_lane] : 0.0;          // an empty slot's likelihood: the row's prior predictive
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
            if constexpr (TOK) {
                if (row_of(r) >= 0) probe_ll[((int64_t)tutt[r] * c.N_max + tpos[r]) * probe_ld + k] = row_ll(r)[k];
            } else
                probe_ll[(int64_t)(i0 + r) * probe_ld + k] = ll[(int64_t)r * KM + k];
        }
        __syncthreads();
    }
    if constexpr (MAP) {
        int moved = 0;
        for (int r = w; r < nr; r += FBI_NT / 64) {         // a wave per item
            const int i = i0 + r;
            if (!consider_unassigned && bt.slot[i] < 0) continue;       // (wave-uniform) keeps -1 and contributes to nothing
            moved += fbi_map_item(bt, pz, ll + (int64_t)r * KM, KM, i, n_new, lane);
        }
        fbi_map_count(moved, w, FBI_NT / 64, lane, n_moved);
        return;
    }
    const double zc_empty = f.lms * log(prior_alpha / (double)KM);
    for (int r = w; r < nr; r += FBI_NT / 64) {             // a wave per item
        if constexpr (TOK) {
            const int64_t e = row_of(r);                    // (wave-uniform)
            if (e < 0) continue;
            const int k = fbb_draw_row(f, bt, KM, prior_alpha, zc_empty, anneal_temp, row_ll(r), sweep, (uint64_t)tutt[r],
                                       (uint64_t)(c.N_max + tpos[r]), lane);
            if (lane == 0) bt.slot[e] = k;
            continue;
        }
        const int i = i0 + r;
        if (!consider_unassigned && bt.slot[i] < 0) continue;           // (wave-uniform) keeps -1 and contributes to nothing
        const int k = fbb_draw_row(f, bt, KM, prior_alpha, zc_empty, anneal_temp, ll + (int64_t)r * KM, sweep, (uint64_t)i, 1ull, lane);
        if (lane == 0) {
            bt.slot[i] = k;
            n_new[i] = 1;
        }
    }
}

// ---------------------------------------------------------------------------------------
// k_fbi_assign_diag32<XT>: the item step with the Student-t terms of diagonal components in float32 on the hardware logarithm
// (FBGMM(..., sync="batch", score_precision="f32"); segk_fbi_assign_diag32).  A sibling of k_fbi_assign<XT, 1>, not a further
// template axis of it: the fp64 forms keep their code.  Only the likelihood half differs:
//   * the tile's rows are staged as float(X[i][d] - centre[d]) (the difference in fp64), the slots' (float(mean - centre),
//     float(q)) pairs come from bt.tab32 (segk_fbb_prepare wrote them), FBI32_KC = 32 slots per pass, two side by side per wave
//     (one LDS read of x per dimension for the two, the pairs as 8-byte broadcasts);
//   * per (item, slot) acc += fbb_term32(m, q, x), dimensions ascending -- the term of fbb_accumulate_rows32 -- then
//     ll = lconst - half * (ln 2 * acc) in fp64; an empty slot keeps prior_rows[i].
// The logits stay fp64 and the draw half is k_fbi_assign's: fbb_draw_row on them, a wave per item.
// Sixteen waves, not k_fbi_assign's eight: with the logarithms on the hardware the draw half (fp64 exp / log per slot and the
// inverse-CDF walk, a chain of dependent steps per item) is most of the kernel, and a wave walks four of the tile's items in a
// row instead of eight.  N = 100 000, D = 39, K_max = 100, B = S = 8: 63.9 us per step with 512 threads (four slots per wave),
// 52 with 1 024; the sweep 0.80 -> 0.71 ms.  92 VGPRs: the sixteen waves are four per SIMD of the five the registers allow, so
// the smaller LDS image buys the second eight waves inside the workgroup, not a second workgroup (200 tiles a step on 256 CUs).
// LDS: fbi32_stage_bytes(D) = 516 D rounded up to 16 (pairs [32][D] of 8 bytes, rows [D][65] floats: the row stride 65 puts
// the staging stores of consecutive dimensions in consecutive banks), then the logits [64][K_max | 1] doubles (the odd row
// stride spreads a wave's 64 stores of one slot over the banks; at K_max = 100 a stride of 100 doubles put them on four) where
// both fit in FBI_LDS_MAX, else in the bounded workspace as for k_fbi_assign.  D = 39, K_max = 100: 71 840 bytes.
// ---------------------------------------------------------------------------------------
#define FBI32_NT 1024                             // threads: sixteen waves over the slots (likelihoods), over the items (draws)
#define FBI32_KW 2                                // slots a wave accumulates side by side
#define FBI32_KC (FBI32_KW * (FBI32_NT / 64))       // slots staged per pass
#define FBI32_XS (FBI_T + 1)                      // floats between the staged rows' dimensions

static __host__ __device__ __forceinline__ size_t fbi32_stage_bytes(int D)
{
    return ((2 * (size_t)FBI32_KC * D + (size_t)FBI32_XS * D) * sizeof(float) + 15) & ~(size_t)15;
}
// doubles between the logit rows of a tile
static __host__ __device__ __forceinline__ int fbi32_ldl(int KM) { return KM | 1; }

// TOK = false: the items of the stand-alone model; TOK = true: the tokens of a segmenter's cell through the lists `L`, the axis
// of k_fbi_assign (segk_fbt_assign_diag32; the float32 inner sweeps of am_sweep(..., score_precision="f32")): the rows are
// gathered through L.row, an entry that names no row of the corpus is staged as zeros and left alone, the draw of token t of
// utterance i uses u01(seed, sweep, i, N_max + t), only bt.slot is written (n_new / new_tok are read by k_fbt_compact alone)
// MAP (items only; k_fbi_assign_map_diag32, segk_fbi_assign_map_diag32): the MAP half of k_fbi_assign on these logits -- pz the
// 65th row of the tile's logits [FBI_T + 1][K_max | 1], fbi_map_item per item, the moved items counted into *n_moved.
// The body of both kernels (smem: the workgroup's dynamic LDS):
template <typename XT, bool TOK, bool MAP>
static __device__ __forceinline__ void fbi_assign_diag32_tile(char *smem, const segk_corpus &c, const segk_fbgmm &f, const segk_fbatch &bt,
                                                              const FbbMap &map, int wg0, int b, uint64_t sweep, double prior_alpha,
                                                              double anneal_temp, int consider_unassigned, int32_t *n_new, double *zbuf,
                                                              double *probe_ll, int64_t probe_ld, const FbtList &L, int32_t *n_moved)
{
    static_assert(!(TOK && MAP), "the MAP half exists for items");
    const int D = c.D, KM = f.K_max, ldl = fbi32_ldl(KM), tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);        // (wave-uniform, and known to be)
    int s, idx;
    if (!fbb_locate(map, wg0 + blockIdx.x, &s, &idx)) return;
    const int slice = map.lo[s];
    const int u0 = bt.utt_range[(slice * bt.n_blocks + b) * 2], u1 = bt.utt_range[(slice * bt.n_blocks + b) * 2 + 1];
    int i0, nr;
    const int32_t *trow = nullptr, *tutt = nullptr, *tpos = nullptr;    // TOK: the tile's entries of the token lists
    if constexpr (TOK) {
        const int n_tok = L.count[s];
        i0 = idx * FBI_T;                                   // the tile's first token of the cell's list
        if (i0 >= n_tok) return;                            // (workgroup-uniform: the grid is sized from the host's bound)
        nr = n_tok - i0 < FBI_T ? n_tok - i0 : FBI_T;
        trow = L.row + L.off[s] + i0;
        tutt = L.utt + L.off[s] + i0;
        tpos = L.pos + L.off[s] + i0;
    } else {
        i0 = u0 + idx * FBI_T;                              // the tile's first item
        if (i0 >= u1) return;                               // a tile beyond its cell's count (workgroup-uniform)
        nr = u1 - i0 < FBI_T ? u1 - i0 : FBI_T;
    }
    // the embedding row of the tile's entry r (TOK: -1 where the list names none -- such an entry is left alone)
    auto row_of = [&](int r) -> int64_t {
        if constexpr (TOK) {
            const int64_t e = trow[r];
            return e >= 0 && e < c.n_emb ? e : -1;
        } else
            return i0 + r;
    };
    float2 *pm = (float2 *)smem;                            // [FBI32_KC][D]: (mean - centre, q) of the staged slots
    float *xs = (float *)(pm + (size_t)FBI32_KC * D);       // [D][FBI32_XS]: the lanes' centred rows side by side
    // [FBI_T][ldl], with MAP a further row: pz
    double *ll = zbuf ? zbuf + (int64_t)blockIdx.x * (FBI_T + (MAP ? 1 : 0)) * ldl : (double *)(smem + fbi32_stage_bytes(D));
    double *pz = nullptr;
    if constexpr (MAP) {                                    // (published by the barriers of the likelihood loop)
        pz = ll + (int64_t)FBI_T * ldl;
        for (int k = tid; k < KM; k += FBI32_NT) pz[k] = log(prior_alpha / (double)KM + bt.cnt[k]);         // fbgmm.py:475-479
    }
    const XT *X = (const XT *)c.X;
    for (int j = tid; j < FBI_T * D; j += FBI32_NT) {
        const int r = j / D, d = j - r * D;
        const int64_t e = r < nr ? row_of(r) : -1;
        xs[d * FBI32_XS + r] = e >= 0 ? (float)((double)X[e * c.ldx + d] - bt.centre[d]) : 0.f;
    }
    const int64_t e_lane = lane < nr ? row_of(lane) : -1;
    const bool valid = e_lane >= 0;
    const double lp = valid ? bt.prior_rows[e_lane] : 0.0;             // an empty slot's likelihood: the row's prior predictive
    const float *tm = bt.tab32, *tq = bt.tab32 + (int64_t)D * KM;
    for (int k0 = 0; k0 < KM; k0 += FBI32_KC) {
        __syncthreads();                                    // (the rows are staged; the previous pass has read its parameters)
        for (int j = tid; j < FBI32_KC * D; j += FBI32_NT) {
            const int kk = j % FBI32_KC, d = j / FBI32_KC, k = k0 + kk;
            pm[kk * D + d] = k < KM ? make_float2(tm[(int64_t)d * KM + k], tq[(int64_t)d * KM + k]) : make_float2(0.f, 0.f);
        }
        __syncthreads();
        const int kw = k0 + w * FBI32_KW;                   // this wave's slots kw .. kw + FBI32_KW - 1 (wave-uniform)
        bool occ[FBI32_KW];
        float acc[FBI32_KW];
        bool any = false;
#pragma unroll
        for (int j = 0; j < FBI32_KW; j++) {
            occ[j] = kw + j < KM && bt.cnt[kw + j] > 0.0;
            acc[j] = 0.f;
            any = any || occ[j];
        }
        if (any) {
            // all four slots, occupied or not (an empty slot's tables are finite -- the prior's -- and a slot beyond K_max is
            // staged as zeros; their sums are dropped below): a test per slot inside the loop made every term wait for its own
            // LDS read
            const float2 *pw = pm + (size_t)(w * FBI32_KW) * D;
#pragma unroll 4
            for (int d = 0; d < D; d++) {
                const float x = xs[d * FBI32_XS + lane];
#pragma unroll
                for (int j = 0; j < FBI32_KW; j++) {
                    const float2 mq = pw[j * D + d];
                    acc[j] += fbb_term32(mq.x, mq.y, x);
                }
            }
        }
        if (valid) {
#pragma unroll
            for (int j = 0; j < FBI32_KW; j++) {
                const int k = kw + j;
                if (k >= KM) continue;
                ll[(int64_t)lane * ldl + k] = occ[j] ? bt.lconst[k] - bt.half[k] * (0.6931471805599453 * (double)acc[j]) : lp;
            }
        }
    }
    __syncthreads();
    if (probe_ll) {             // the likelihood part of the logits, as the draws below use it: the rows of the items they take
        for (int j = tid; j < nr * KM; j += FBI32_NT) {
            const int r = j / KM, k = j - r * KM;
            if constexpr (TOK) {
                if (row_of(r) >= 0) probe_ll[((int64_t)tutt[r] * c.N_max + tpos[r]) * probe_ld + k] = ll[(int64_t)r * ldl + k];
            } else if (consider_unassigned || bt.slot[i0 + r] >= 0)
                probe_ll[(int64_t)(i0 + r) * probe_ld + k] = ll[(int64_t)r * ldl + k];
        }
        __syncthreads();
    }
    if constexpr (MAP) {
        int moved = 0;
        for (int r = w; r < nr; r += FBI32_NT / 64) {       // a wave per item
            const int i = i0 + r;
            if (!consider_unassigned && bt.slot[i] < 0) continue;       // (wave-uniform) keeps -1 and contributes to nothing
            moved += fbi_map_item(bt, pz, ll + (int64_t)r * ldl, KM, i, n_new, lane);
        }
        fbi_map_count(moved, w, FBI32_NT / 64, lane, n_moved);
        return;
    }
    const double zc_empty = f.lms * log(prior_alpha / (double)KM);
    for (int r = w; r < nr; r += FBI32_NT / 64) {             // a wave per item
        if constexpr (TOK) {
            const int64_t e = row_of(r);                    // (wave-uniform)
            if (e < 0) continue;
            const int k = fbb_draw_row(f, bt, KM, prior_alpha, zc_empty, anneal_temp, ll + (int64_t)r * ldl, sweep, (uint64_t)tutt[r],
                                       (uint64_t)(c.N_max + tpos[r]), lane);
            if (lane == 0) bt.slot[e] = k;
            continue;
        }
        const int i = i0 + r;
        if (!consider_unassigned && bt.slot[i] < 0) continue;           // (wave-uniform) keeps -1 and contributes to nothing
        const int k = fbb_draw_row(f, bt, KM, prior_alpha, zc_empty, anneal_temp, ll + (int64_t)r * ldl, sweep, (uint64_t)i, 1ull, lane);
        if (lane == 0) {
            bt.slot[i] = k;
            n_new[i] = 1;
        }
    }
}

template <typename XT, bool TOK = false>
__global__ __launch_bounds__(FBI32_NT) void k_fbi_assign_diag32(segk_corpus c, segk_fbgmm f, segk_fbatch bt, FbbMap map, int wg0, int b,
                                                             uint64_t sweep, double prior_alpha, double anneal_temp,
                                                             int consider_unassigned, int32_t *n_new, double *zbuf, double *probe_ll,
                                                             int64_t probe_ld, FbtList L)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fbi_assign_diag32_tile<XT, TOK, false>(smem, c, f, bt, map, wg0, b, sweep, prior_alpha, anneal_temp, consider_unassigned, n_new, zbuf,
                                           probe_ll, probe_ld, L, nullptr);
}

template <typename XT>
__global__ __launch_bounds__(FBI32_NT) void k_fbi_assign_map_diag32(segk_corpus c, segk_fbgmm f, segk_fbatch bt, FbbMap map, int wg0,
                                                                 int b, double prior_alpha, int consider_unassigned, int32_t *n_new,
                                                                 double *zbuf, double *probe_ll, int64_t probe_ld, int32_t *n_moved)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    fbi_assign_diag32_tile<XT, false, true>(smem, c, f, bt, map, wg0, b, 0, prior_alpha, 1.0, consider_unassigned, n_new, zbuf, probe_ll,
                                            probe_ld, FbtList{}, n_moved);
}

// What both entry points do once their arguments are checked: the tiles of block b mapped to workgroups (m: FBI_T entries
// each), with cov_type 2 the token-likelihood table formed, the logits placed (LDS, or the bounded workspace and several
// launches), the launches.  tok: the lists of segk_fbt_assign (NULL: items).  n_moved (items only): the MAP half in place of
// the draws -- the tile's logits are then FBI_T + 1 rows, the last one the prior terms pz, and the same placement rule holds for
// the 65 rows (cov_type 2: pz alone, K_max <= 1024 doubles of LDS).
static int32_t fbi_launch(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, const FbbMap &m, int32_t s_lo,
                          int32_t s_n, int32_t b, const int32_t *n_utts, int most, uint64_t sweep, double anneal_temp,
                          int32_t consider_unassigned, const int32_t *new_tok, int32_t *n_new, double *probe_ll, int64_t probe_ld,
                          const FbtList *tok, void *stream, int32_t *n_moved = nullptr)
{
    const int n_wg = m.off[s_n];
    hipStream_t st = (hipStream_t)stream;
    const double *fc_ll = nullptr;
    int fc_ucap = 0;
    size_t lds = 0;
    int per_launch = n_wg;
    double *zbuf = nullptr;
    const int rows = FBI_T + (n_moved ? 1 : 0);             // rows of a tile's logits
    if (f->cov_type == 2) {
        if (!tok && consider_unassigned) {
            hipLaunchKernelGGL(k_fbi_mark, dim3((unsigned)((most + 255) / 256), (unsigned)s_n), dim3(256), 0, st, *bt, s_lo, b, n_new);
            SEGK_LAUNCH_CHECK();
        }
        if (int rc = segk_fcb_token_ll(ctx, c, f, bt, s_lo, s_n, b, n_utts, new_tok, n_new, &fc_ll, &fc_ucap, stream)) return rc;
        if (n_moved) lds = (size_t)f->K_max * sizeof(double);
    } else {
        const size_t stage = fbi_stage_doubles(c->D) * sizeof(double), tile = (size_t)rows * f->K_max * sizeof(double);
        SEGK_REQUIRE(stage <= FBI_LDS_MAX, "the rows and the staged slots of a tile do not fit in LDS");
        if (stage + tile <= FBI_LDS_MAX) {
            lds = stage + tile;
        } else {
            lds = stage;
            const int mib = segk_env_int("SEGK_FBI_Z_MIB", FBI_Z_MIB);
            const size_t cap = ((size_t)(mib > 0 ? mib : FBI_Z_MIB) << 20) / tile;
            per_launch = cap < 1 ? 1 : (cap < (size_t)n_wg ? (int)cap : n_wg);
            const int64_t need = (int64_t)per_launch * rows * f->K_max;
            if (int rc = segk_ws_grow(ctx, &ctx->fbi_z, &ctx->fbi_z_n, need, (size_t)need * sizeof(double), st)) return rc;
            zbuf = ctx->fbi_z;
        }
    }
    const FbtList none = {};
#define SEGK_FBI(XT, COV, TOK, MAP)                                                                                             \
    do {                                                                                                                        \
        SEGK_CHECK_HIP(segk_dyn_lds((const void *)k_fbi_assign<XT, COV, TOK, MAP>, lds));                                       \
        for (int wg0 = 0; wg0 < n_wg; wg0 += per_launch) {                                                                      \
            const int n = n_wg - wg0 < per_launch ? n_wg - wg0 : per_launch;                                                    \
            hipLaunchKernelGGL((k_fbi_assign<XT, COV, TOK, MAP>), dim3((unsigned)n), dim3(FBI_NT), lds, st, *c, *f, *bt, m, wg0, \
                               b, sweep, f->alpha, anneal_temp, consider_unassigned ? 1 : 0, n_new, zbuf, fc_ll, fc_ucap,       \
                               probe_ll, probe_ld, tok ? *tok : none, n_moved);                                                 \
        }                                                                                                                       \
    } while (0)
#define SEGK_FBI_COV(XT, TOK, MAP)                                                                                              \
    do {                                                                                                                        \
        if (f->cov_type == 0) SEGK_FBI(XT, 0, TOK, MAP);                                                                        \
        else if (f->cov_type == 1) SEGK_FBI(XT, 1, TOK, MAP);                                                                   \
        else SEGK_FBI(XT, 2, TOK, MAP);                                                                                         \
    } while (0)
    if (c->x_dtype == SEGK_F32) {
        if (tok) SEGK_FBI_COV(float, true, false);
        else if (n_moved) SEGK_FBI_COV(float, false, true);
        else SEGK_FBI_COV(float, false, false);
    } else {
        if (tok) SEGK_FBI_COV(double, true, false);
        else if (n_moved) SEGK_FBI_COV(double, false, true);
        else SEGK_FBI_COV(double, false, false);
    }
#undef SEGK_FBI_COV
#undef SEGK_FBI
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

// fbi_launch for the float32 form (segk_fbi_assign_diag32 / segk_fbt_assign_diag32): the placement rule with this form's byte
// counts -- the logits in LDS while fbi32_stage_bytes(D) + 512 (K_max | 1) <= FBI_LDS_MAX, else in the bounded workspace of the
// context (SEGK_FBI_Z_MIB) and several launches -- then the launches.  tok: the lists of segk_fbt_assign_diag32 (NULL: items).
// n_moved (items only; segk_fbi_assign_map_diag32): the MAP kernel, 65 rows of K_max | 1 doubles per tile (520 (K_max | 1)
// bytes) under the same rule.
static int32_t fbi32_launch_form(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, const FbbMap &m,
                                 int32_t s_n, int32_t b, uint64_t sweep, double anneal_temp, int32_t consider_unassigned, int32_t *n_new,
                                 double *probe_ll, int64_t probe_ld, const FbtList *tok, void *stream, int32_t *n_moved)
{
    const int n_wg = m.off[s_n];
    hipStream_t st = (hipStream_t)stream;
    const int rows = FBI_T + (n_moved ? 1 : 0);             // rows of a tile's logits: with the MAP half one more, pz
    const size_t stage = fbi32_stage_bytes(c->D), tile = (size_t)rows * fbi32_ldl(f->K_max) * sizeof(double);
    SEGK_REQUIRE(stage <= FBI_LDS_MAX, "the rows and the staged slots of a tile do not fit in LDS");
    size_t lds = stage + tile;
    int per_launch = n_wg;
    double *zbuf = nullptr;
    if (lds > FBI_LDS_MAX) {
        lds = stage;
        const int mib = segk_env_int("SEGK_FBI_Z_MIB", FBI_Z_MIB);
        const size_t cap = ((size_t)(mib > 0 ? mib : FBI_Z_MIB) << 20) / tile;
        per_launch = cap < 1 ? 1 : (cap < (size_t)n_wg ? (int)cap : n_wg);
        const int64_t need = (int64_t)per_launch * rows * fbi32_ldl(f->K_max);
        if (int rc = segk_ws_grow(ctx, &ctx->fbi_z, &ctx->fbi_z_n, need, (size_t)need * sizeof(double), st)) return rc;
        zbuf = ctx->fbi_z;
    }
    const FbtList none = {};
#define SEGK_FBI32(XT, TOK)                                                                                                     \
    do {                                                                                                                        \
        SEGK_CHECK_HIP(segk_dyn_lds((const void *)k_fbi_assign_diag32<XT, TOK>, lds));                                          \
        for (int wg0 = 0; wg0 < n_wg; wg0 += per_launch) {                                                                      \
            const int n = n_wg - wg0 < per_launch ? n_wg - wg0 : per_launch;                                                    \
            hipLaunchKernelGGL((k_fbi_assign_diag32<XT, TOK>), dim3((unsigned)n), dim3(FBI32_NT), lds, st, *c, *f, *bt, m, wg0, \
                               b, sweep, f->alpha, anneal_temp, consider_unassigned ? 1 : 0, n_new, zbuf, probe_ll, probe_ld,   \
                               tok ? *tok : none);                                                                              \
        }                                                                                                                       \
    } while (0)
#define SEGK_FBI32_MAP(XT)                                                                                                      \
    do {                                                                                                                        \
        SEGK_CHECK_HIP(segk_dyn_lds((const void *)k_fbi_assign_map_diag32<XT>, lds));                                           \
        for (int wg0 = 0; wg0 < n_wg; wg0 += per_launch) {                                                                      \
            const int n = n_wg - wg0 < per_launch ? n_wg - wg0 : per_launch;                                                    \
            hipLaunchKernelGGL(k_fbi_assign_map_diag32<XT>, dim3((unsigned)n), dim3(FBI32_NT), lds, st, *c, *f, *bt, m, wg0, b, \
                               f->alpha, consider_unassigned ? 1 : 0, n_new, zbuf, probe_ll, probe_ld, n_moved);                \
        }                                                                                                                       \
    } while (0)
    if (c->x_dtype == SEGK_F32) {
        if (tok) SEGK_FBI32(float, true);
        else if (n_moved) SEGK_FBI32_MAP(float);
        else SEGK_FBI32(float, false);
    } else {
        if (tok) SEGK_FBI32(double, true);
        else if (n_moved) SEGK_FBI32_MAP(double);
        else SEGK_FBI32(double, false);
    }
#undef SEGK_FBI32_MAP
#undef SEGK_FBI32
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

// ... the sampled kernel (segk_fbi_assign_diag32 / segk_fbt_assign_diag32)
static int32_t fbi32_launch(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, const FbbMap &m, int32_t s_n,
                            int32_t b, uint64_t sweep, double anneal_temp, int32_t consider_unassigned, int32_t *n_new,
                            double *probe_ll, int64_t probe_ld, const FbtList *tok, void *stream)
{
    return fbi32_launch_form(ctx, c, f, bt, m, s_n, b, sweep, anneal_temp, consider_unassigned, n_new, probe_ll, probe_ld, tok, stream,
                             nullptr);
}

// what both entry points ask of their arguments beyond the corpus' shape
static int fbi_check(const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, int32_t s_lo, int32_t s_n, int32_t b,
                     const double *probe_ll, int64_t probe_ld, const char *who)
{
    SEGK_REQUIRE(c->x_dtype == SEGK_F32 || c->x_dtype == SEGK_F64, "unsupported dtype");
    SEGK_REQUIRE(f->cov_type >= 0 && f->cov_type <= 2, "cov_type must be 0 (fixed), 1 (diag) or 2 (full)");
    SEGK_REQUIRE(c->D > 0 && c->D <= 256, "batch mode supports D <= 256");
    SEGK_REQUIRE(f->K_max >= 1 && f->K_max <= 8192, "K_max");
    SEGK_REQUIRE(bt->n_slices >= 1 && bt->n_slices <= 16 && bt->n_blocks >= 1, "slices / blocks");
    SEGK_REQUIRE(s_lo >= 0 && s_n >= 1 && s_n <= 16 && s_lo + s_n <= bt->n_slices && b >= 0 && b < bt->n_blocks, "slice / block range");
    SEGK_REQUIRE(bt->prior_rows && bt->utt_range && bt->slot && bt->cnt && bt->mean_t && bt->q_t && bt->lconst && bt->half,
                 "batch state (prior_rows, ranges, slot, slot tables)");
    SEGK_REQUIRE(!probe_ll || probe_ld >= f->K_max, "probe leading dimension");
    if (f->cov_type == 2)
        if (int rc = segk_fcb_check(c, f, bt, who)) return rc;
    return SEGK_OK;
}

// the tiles of block b of the local slices mapped to workgroups (FBI_T items each); *most: the items of the largest cell
static int fbi_item_map(const int32_t *n_items, int32_t s_lo, int32_t s_n, FbbMap *m, int *most)
{
    m->n = s_n;
    m->off[0] = 0;
    *most = 0;
    for (int s = 0; s < s_n; s++) {
        SEGK_REQUIRE(n_items[s] >= 0, "item counts");
        m->lo[s] = s_lo + s;
        m->off[s + 1] = m->off[s] + (n_items[s] + FBI_T - 1) / FBI_T;
        *most = n_items[s] > *most ? n_items[s] : *most;
    }
    return SEGK_OK;
}

// the token lists of block b: the tiles mapped to workgroups from the host's bounds, the workspace, k_fbt_compact -- or, with
// `was` (segk_fbi_assign_orphans), k_fbi_orphans: the lists of the block's orphans, n_new marked
static int32_t fbt_lists(segk_ctx *ctx, const segk_corpus *c, const segk_fbatch *bt, int32_t s_lo, int32_t s_n, int32_t b,
                         const int32_t *n_utts, const int32_t *tok_cap, const int32_t *new_tok, int32_t *n_new, FbbMap *mp,
                         FbtList *Lp, void *stream, const int32_t *was = nullptr)
{
    FbbMap &m = *mp;
    FbtList &L = *Lp;
    m.n = s_n;
    m.off[0] = 0;
    L.off[0] = 0;
    for (int s = 0; s < s_n; s++) {
        SEGK_REQUIRE(n_utts[s] >= 0 && n_utts[s] <= c->n_utt, "utterance counts");
        SEGK_REQUIRE(tok_cap[s] >= 0 && (int64_t)tok_cap[s] <= (int64_t)n_utts[s] * c->N_max, "token bounds (the landmarks of the cell)");
        SEGK_REQUIRE((int64_t)L.off[s] + tok_cap[s] < (int64_t)1 << 30, "token bounds of a block");
        m.lo[s] = s_lo + s;
        m.off[s + 1] = m.off[s] + (tok_cap[s] + FBI_T - 1) / FBI_T;
        L.off[s + 1] = L.off[s] + tok_cap[s];
    }
    if (m.off[s_n] == 0) return SEGK_OK;
    const int64_t cap = L.off[s_n], need = 16 + 3 * cap;
    if (int rc = segk_ws_grow(ctx, &ctx->fbt_tok, &ctx->fbt_tok_n, need, (size_t)need * sizeof(int32_t), (hipStream_t)stream)) return rc;
    L.count = ctx->fbt_tok;
    L.row = ctx->fbt_tok + 16;
    L.utt = L.row + cap;
    L.pos = L.utt + cap;
    if (was)
        hipLaunchKernelGGL(k_fbi_orphans, dim3((unsigned)s_n), dim3(FBT_NT), 0, (hipStream_t)stream, *c, *bt, L, s_lo, b, was, n_new);
    else
        hipLaunchKernelGGL(k_fbt_compact, dim3((unsigned)s_n), dim3(FBT_NT), 0, (hipStream_t)stream, *c, *bt, L, s_lo, b, new_tok, n_new);
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

// ---------------------------------------------------------------------------------------
// FBGMM.predict / score_samples / predict_log_proba (segk_fbi_predict, segk_fbi_predict_diag32; specification
// tests/fbgmm_predict.py): query rows that are not in the model, scored against the statistics of ALL items that hold a slot
// (the state segk_fbb_prepare(-1) leaves) -- an unassigned item appended to X, as fbgmm.py:256-285 (log_marg_i), :436-445 (the
// logits of gibbs_sample_inside_loop_i) and :475-491 (map_assign_i) see it.  Nothing of the model is written.
//
//   k_fbi_predict<XT, COV>     the tile of k_fbi_assign -- 64 query rows per workgroup, a lane each, eight waves over the slots --
//                              and, for cov_type 0 / 1, a SIBLING of its likelihood half, operation for operation (rows staged
//                              fp64 [D][64], 16 slots' (mean, q) per pass, dimensions ascending, lconst - half acc, an empty slot
//                              the row's prior predictive), so the bits are those a batch sweep forms for the same row and
//                              statistics.  The existing instantiations keep their code.  cov_type 2: the epilogue alone, over the
//                              table k_fcb_token_ll formed on a view of the query rows.
//   k_fbi_predict_diag32<XT>   the likelihood half of k_fbi_assign_diag32 (fbb_term32, float32 rows and tables, sixteen waves),
//                              logit rows of K_max | 1 doubles, the same fp64 epilogue.
//   epilogue, a wave per row   label: fbb_map_row on pz[k] = log(alpha / K_max + n_k) (no lms), renumbered to the reference's
//                              view -- an occupied slot its rank among the occupied slots, an empty one K --; density: the
//                              wave's maximum of t_k = lms pz[k] - lms log(N_a + alpha) + ll[k], exp(t_k - max) summed per lane
//                              over k = lane, lane + 64, ..., then fb_wave_sum (a fixed order: the value does not depend on
//                              the launch shape); log_resp[k] = t_k - density (the constant cancels), slot order.
// LDS: the staged rows and slots of the sibling, then pz [K_max] doubles, the logits where they fit, the rank table [K_max + 1]
// ints (the last entry K).  A plain grid of independent workgroups: no atomic, no barrier across workgroups.
// ---------------------------------------------------------------------------------------
static __host__ __device__ __forceinline__ size_t fbi_predict_rank_bytes(int KM) { return (((size_t)KM + 1) * sizeof(int32_t) + 7) & ~(size_t)7; }
// bytes of a workgroup beside its logits, fp64 form (COV 2: the two tables alone) and float32 form
static __host__ __device__ __forceinline__ size_t fbi_predict_fixed_bytes(int D, int KM, bool fullcov)
{
    return (fullcov ? 0 : fbi_stage_doubles(D) * sizeof(double)) + (size_t)KM * sizeof(double) + fbi_predict_rank_bytes(KM);
}
static __host__ __device__ __forceinline__ size_t fbi32_predict_fixed_bytes(int D, int KM)
{
    return fbi32_stage_bytes(D) + (size_t)KM * sizeof(double) + fbi_predict_rank_bytes(KM);
}

// the workgroup's tables: the prior terms of the label, and per slot the number of occupied slots before it (wave 0: a ballot
// per 64 slots); the caller's barrier publishes them
static __device__ __forceinline__ void fbi_predict_tables(const segk_fbatch &bt, int KM, double prior_alpha, double *pz, int32_t *rank, int tid,
                                                          int nt)
{
    for (int k = tid; k < KM; k += nt) pz[k] = log(prior_alpha / (double)KM + bt.cnt[k]);                   // fbgmm.py:475-479
    if (tid < 64) {
        int run = 0;
        for (int k0 = 0; k0 < KM; k0 += 64) {
            const int k = k0 + tid;
            const bool occ = k < KM && bt.cnt[k] > 0.0;
            const unsigned long long m = __ballot(occ);
            if (k < KM) rank[k] = run + __popcll(m & ((1ull << tid) - 1ull));
            run += __popcll(m);
        }
        if (tid == 0) rank[KM] = run;
    }
}

// the epilogue: rows r = w, w + nw, ... of the tile, a wave each; ll: the tile's likelihoods, ldl doubles between rows (read only)
static __device__ __forceinline__ void fbi_predict_rows(const segk_fbgmm &f, const segk_fbatch &bt, int KM, double prior_alpha, const double *pz,
                                                        const int32_t *rank, const double *ll, int64_t ldl, int nr, int64_t out0, int w,
                                                        int nw, int lane, int32_t *label, double *log_density, double *log_resp,
                                                        int64_t resp_ld)
{
    const double lms = f.lms, lt = lms * log(bt.scal[0] + prior_alpha);     // fbgmm.py:268-272
    for (int r = w; r < nr; r += nw) {
        const double *zr = ll + (int64_t)r * ldl;
        const int64_t i = out0 + r;
        if (label) {
            const int k = fbb_map_row(pz, zr, KM, lane);    // fbgmm.py:475-488
            if (lane == 0) label[i] = bt.cnt[k] > 0.0 ? rank[k] : rank[KM];                                   // :489-490
        }
        if (!log_density && !log_resp) continue;
        auto t_of = [&](int k) -> double { return lms * pz[k] - lt + zr[k]; };
        double mx = NEG_INF_D;
        for (int k = lane; k < KM; k += 64) {
            const double v = t_of(k);
            mx = v > mx ? v : mx;
        }
        mx = fb_wave_max(mx, false);
        double sv = 0.0;
        for (int k = lane; k < KM; k += 64) sv += exp(t_of(k) - mx);
        const double dens = log(fb_wave_sum(sv)) + mx;
        if (log_density && lane == 0) log_density[i] = dens;
        if (log_resp)
            for (int k = lane; k < KM; k += 64) log_resp[i * resp_ld + k] = t_of(k) - dens;
    }
}

// cq: a view of the query rows of this launch (X its first row, n_emb their number); out0: the index of that row in the
// caller's arrays.  zbuf: the launch's logits where they do not fit in LDS.  fc_ll (COV 2): row r of the view at fc_ll + r K_max.
template <typename XT, int COV>
__global__ __launch_bounds__(FBI_NT) void k_fbi_predict(segk_corpus cq, segk_fbgmm f, segk_fbatch bt, int64_t out0, double prior_alpha,
                                                       const double *prior_rows_q, double *zbuf, const double *fc_ll, int32_t *label,
                                                       double *log_density, double *log_resp, int64_t resp_ld, double *probe_ll,
                                                       int64_t probe_ld)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int D = cq.D, KM = f.K_max, tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);        // (wave-uniform, and known to be)
    const int64_t i0 = (int64_t)blockIdx.x * FBI_T;
    if (i0 >= cq.n_emb) return;                             // a tile at or beyond the rows (workgroup-uniform)
    const int nr = cq.n_emb - i0 < FBI_T ? (int)(cq.n_emb - i0) : FBI_T;
    double *pz;
    int32_t *rank;
    const double *ll;
    if constexpr (COV == 2) {
        pz = (double *)smem;
        rank = (int32_t *)(pz + KM);
        fbi_predict_tables(bt, KM, prior_alpha, pz, rank, tid, FBI_NT);
        ll = fc_ll + i0 * KM;
        __syncthreads();
    } else {
        double *xs = (double *)smem;                        // [D][FBI_T]: the lanes' rows side by side
        double *pm = xs + (size_t)FBI_T * D;                // [FBI_KC][D][2]: (mean, q) of the staged slots
        pz = pm + 2 * (size_t)FBI_KC * D;
        double *lw = zbuf ? zbuf + (int64_t)blockIdx.x * FBI_T * KM : pz + KM;
        rank = (int32_t *)(zbuf ? pz + KM : pz + KM + (size_t)FBI_T * KM);
        fbi_predict_tables(bt, KM, prior_alpha, pz, rank, tid, FBI_NT);     // (published by the barriers of the likelihood loop)
        const XT *X = (const XT *)cq.X;
        for (int j = tid; j < FBI_T * D; j += FBI_NT) {
            const int r = j / D, d = j - r * D;
            xs[d * FBI_T + r] = r < nr ? (double)X[(i0 + r) * cq.ldx + d] : 0.0;
        }
        const bool valid = lane < nr;
        const double lp = valid ? prior_rows_q[out0 + i0 + lane] : 0.0;         // an empty slot's likelihood: the row's prior predictive
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
                    lw[(int64_t)lane * KM + k] = occ[j] ? bt.lconst[k] - bt.half[k] * acc[j] : lp;
                }
            }
        }
        __syncthreads();
        ll = lw;
    }
    if (probe_ll)               // the likelihood part of the logits, as the epilogue uses it
        for (int j = tid; j < nr * KM; j += FBI_NT) {
            const int r = j / KM, k = j - r * KM;
            probe_ll[(out0 + i0 + r) * probe_ld + k] = ll[(int64_t)r * KM + k];
        }
    fbi_predict_rows(f, bt, KM, prior_alpha, pz, rank, ll, KM, nr, out0 + i0, w, FBI_NT / 64, lane, label, log_density, log_resp, resp_ld);
}

template <typename XT>
__global__ __launch_bounds__(FBI32_NT) void k_fbi_predict_diag32(segk_corpus cq, segk_fbgmm f, segk_fbatch bt, int64_t out0,
                                                              double prior_alpha, const double *prior_rows_q, double *zbuf,
                                                              int32_t *label, double *log_density, double *log_resp, int64_t resp_ld,
                                                              double *probe_ll, int64_t probe_ld)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int D = cq.D, KM = f.K_max, ldl = fbi32_ldl(KM), tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);        // (wave-uniform, and known to be)
    const int64_t i0 = (int64_t)blockIdx.x * FBI_T;
    if (i0 >= cq.n_emb) return;                             // a tile at or beyond the rows (workgroup-uniform)
    const int nr = cq.n_emb - i0 < FBI_T ? (int)(cq.n_emb - i0) : FBI_T;
    float2 *pm = (float2 *)smem;                            // [FBI32_KC][D]: (mean - centre, q) of the staged slots
    float *xs = (float *)(pm + (size_t)FBI32_KC * D);       // [D][FBI32_XS]: the lanes' centred rows side by side
    double *pz = (double *)(smem + fbi32_stage_bytes(D));
    double *ll = zbuf ? zbuf + (int64_t)blockIdx.x * FBI_T * ldl : pz + KM;         // [FBI_T][ldl]
    int32_t *rank = (int32_t *)(zbuf ? pz + KM : pz + KM + (size_t)FBI_T * ldl);
    fbi_predict_tables(bt, KM, prior_alpha, pz, rank, tid, FBI32_NT);       // (published by the barriers of the likelihood loop)
    const XT *X = (const XT *)cq.X;
    for (int j = tid; j < FBI_T * D; j += FBI32_NT) {
        const int r = j / D, d = j - r * D;
        xs[d * FBI32_XS + r] = r < nr ? (float)((double)X[(i0 + r) * cq.ldx + d] - bt.centre[d]) : 0.f;
    }
    const bool valid = lane < nr;
    const double lp = valid ? prior_rows_q[out0 + i0 + lane] : 0.0;        // an empty slot's likelihood: the row's prior predictive
    const float *tm = bt.tab32, *tq = bt.tab32 + (int64_t)D * KM;
    for (int k0 = 0; k0 < KM; k0 += FBI32_KC) {
        __syncthreads();                                    // (the rows are staged; the previous pass has read its parameters)
        for (int j = tid; j < FBI32_KC * D; j += FBI32_NT) {
            const int kk = j % FBI32_KC, d = j / FBI32_KC, k = k0 + kk;
            pm[kk * D + d] = k < KM ? make_float2(tm[(int64_t)d * KM + k], tq[(int64_t)d * KM + k]) : make_float2(0.f, 0.f);
        }
        __syncthreads();
        const int kw = k0 + w * FBI32_KW;                   // this wave's slots kw .. kw + FBI32_KW - 1 (wave-uniform)
        bool occ[FBI32_KW];
        float acc[FBI32_KW];
        bool any = false;
#pragma unroll
        for (int j = 0; j < FBI32_KW; j++) {
            occ[j] = kw + j < KM && bt.cnt[kw + j] > 0.0;
            acc[j] = 0.f;
            any = any || occ[j];
        }
        if (any) {
            const float2 *pw = pm + (size_t)(w * FBI32_KW) * D;
#pragma unroll 4
            for (int d = 0; d < D; d++) {
                const float x = xs[d * FBI32_XS + lane];
#pragma unroll
                for (int j = 0; j < FBI32_KW; j++) {
                    const float2 mq = pw[j * D + d];
                    acc[j] += fbb_term32(mq.x, mq.y, x);
                }
            }
        }
        if (valid) {
#pragma unroll
            for (int j = 0; j < FBI32_KW; j++) {
                const int k = kw + j;
                if (k >= KM) continue;
                ll[(int64_t)lane * ldl + k] = occ[j] ? bt.lconst[k] - bt.half[k] * (0.6931471805599453 * (double)acc[j]) : lp;
            }
        }
    }
    __syncthreads();
    if (probe_ll)               // the likelihood part of the logits, as the epilogue uses it
        for (int j = tid; j < nr * KM; j += FBI32_NT) {
            const int r = j / KM, k = j - r * KM;
            probe_ll[(out0 + i0 + r) * probe_ld + k] = ll[(int64_t)r * ldl + k];
        }
    fbi_predict_rows(f, bt, KM, prior_alpha, pz, rank, ll, ldl, nr, out0 + i0, w, FBI32_NT / 64, lane, label, log_density, log_resp,
                     resp_ld);
}

// the tables of the view of the query rows k_fcb_token_ll walks (cov_type 2): one cell [0, n) of one slice and one block, row i
// its own one-landmark utterance with one token
__global__ __launch_bounds__(256) void k_fbi_predict_view(int32_t *range, int32_t *new_tok, int32_t *n_new, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        range[0] = 0;
        range[1] = n;
    }
    if (i < n) {
        new_tok[i] = i;
        n_new[i] = 1;
    }
}

// a view of the query rows [r0, r0 + n) as a corpus of items
static segk_corpus fbi_query_view(const segk_corpus *c, const void *Xq, int64_t ldq, int64_t r0, int64_t n)
{
    segk_corpus v = {};
    const size_t es = c->x_dtype == SEGK_F32 ? sizeof(float) : sizeof(double);
    v.X = (const char *)Xq + (size_t)r0 * (size_t)ldq * es;
    v.x_dtype = c->x_dtype;
    v.D = c->D;
    v.n_emb = n;
    v.ldx = ldq;
    v.n_utt = (int32_t)n;
    v.N_max = 1;
    return v;
}

// what both predict entry points ask of their arguments; *done: nothing to launch
static int fbi_predict_check(const segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, const void *Xq,
                             int64_t ldq, int64_t M, const double *prior_rows_q, const double *log_resp, int64_t resp_ld,
                             const double *probe_ll, int64_t probe_ld, const char *who, bool *done)
{
    *done = false;
    SEGK_REQUIRE(ctx && c && f && bt, "NULL argument");
    if (f->lm_unigram) {
        segk_set_error("%s: held-out rows are scored by the stand-alone mixture model, which takes no language model", who);
        return SEGK_ERR_UNSUPPORTED;
    }
    SEGK_REQUIRE(!c->vec_ids && !c->band_ids, "a corpus of items: no span tables");
    SEGK_REQUIRE(c->x_dtype == SEGK_F32 || c->x_dtype == SEGK_F64, "unsupported dtype");
    SEGK_REQUIRE(f->cov_type >= 0 && f->cov_type <= 2, "cov_type must be 0 (fixed), 1 (diag) or 2 (full)");
    SEGK_REQUIRE(c->D > 0 && c->D <= 256, "batch mode supports D <= 256");
    SEGK_REQUIRE(f->K_max >= 1 && f->K_max <= 8192, "K_max");
    SEGK_REQUIRE(M >= 0 && M < ((int64_t)1 << 31), "query rows");
    SEGK_REQUIRE(bt->cnt && bt->mean_t && bt->q_t && bt->lconst && bt->half && bt->scal,
                 "batch state (the slot tables and totals segk_fbb_prepare(-1) writes)");
    SEGK_REQUIRE(!log_resp || resp_ld >= f->K_max, "log_resp leading dimension");
    SEGK_REQUIRE(!probe_ll || probe_ld >= f->K_max, "probe leading dimension");
    if (f->cov_type == 2) {
        segk_fbatch with_rows = *bt;                        // (segk_fcb_check asks for prior rows: the query's stand for them)
        with_rows.prior_rows = const_cast<double *>(prior_rows_q ? prior_rows_q : bt->prior_rows);
        if (int rc = segk_fcb_check(c, f, &with_rows, who)) return rc;
    }
    if (M == 0) {
        *done = true;
        return SEGK_OK;
    }
    SEGK_REQUIRE(Xq && ldq >= c->D, "query rows (Xq, ldq)");
    SEGK_REQUIRE(prior_rows_q, "prior_rows_q: M doubles of workspace");
    return SEGK_OK;
}

// the prior predictive of every query row (an empty slot's likelihood) into prior_rows_q
static int fbi_predict_prior_rows(const segk_corpus *c, const segk_fbgmm *f, const void *Xq, int64_t ldq, int64_t M, double *prior_rows_q,
                                  void *stream)
{
    const segk_corpus v = fbi_query_view(c, Xq, ldq, 0, M);
    if (f->cov_type == 2) return segk_fc_prior_rows_view(&v, f, prior_rows_q, stream);
    return segk_fbb_prior_rows(nullptr, &v, f, prior_rows_q, stream);
}

// tiles of a launch and the workspace of their logits, where a tile's do not fit in LDS beside `fixed` bytes
static int fbi_predict_place(segk_ctx *ctx, size_t fixed, size_t tile, int n_tiles, size_t *lds, int *per_launch, double **zbuf, hipStream_t st)
{
    SEGK_REQUIRE(fixed <= FBI_LDS_MAX, "the rows and the staged slots of a tile do not fit in LDS");
    *per_launch = n_tiles;
    *zbuf = nullptr;
    if (fixed + tile <= FBI_LDS_MAX) {
        *lds = fixed + tile;
        return SEGK_OK;
    }
    *lds = fixed;
    const size_t cap = segk_env_mib("SEGK_FBI_Z_MIB", FBI_Z_MIB) / tile;
    *per_launch = cap < 1 ? 1 : (cap < (size_t)n_tiles ? (int)cap : n_tiles);
    const int64_t need = (int64_t)*per_launch * (int64_t)(tile / sizeof(double));
    if (int rc = segk_ws_grow(ctx, &ctx->fbi_z, &ctx->fbi_z_n, need, (size_t)need * sizeof(double), st)) return rc;
    *zbuf = ctx->fbi_z;
    return SEGK_OK;
}

extern "C" {

int32_t segk_fbi_predict(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, const void *Xq,
                         int64_t ldq, int64_t M, double *prior_rows_q, int32_t *label, double *log_density, double *log_resp,
                         int64_t resp_ld, double *probe_ll, int64_t probe_ld, void *stream)
{
    bool done;
    if (int rc = fbi_predict_check(ctx, c, f, bt, Xq, ldq, M, prior_rows_q, log_resp, resp_ld, probe_ll, probe_ld, "segk_fbi_predict", &done))
        return rc;
    if (done) return SEGK_OK;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = fbi_predict_prior_rows(c, f, Xq, ldq, M, prior_rows_q, stream)) return rc;
    const int KM = f->K_max;
    if (f->cov_type == 2) {
        // the second form: the likelihood table by k_fcb_token_ll on a view of a chunk of the query, then the epilogue kernel.
        // The chunks keep the table within the bound of the logits' workspace (SEGK_FBI_Z_MIB)
        int64_t ch = (int64_t)((segk_env_mib("SEGK_FBI_Z_MIB", FBI_Z_MIB) / ((size_t)KM * sizeof(double))) / FBI_T) * FBI_T;
        ch = ch < FBI_T ? FBI_T : ch;
        ch = ch > M ? M : ch;
        const int64_t need = 2 + 2 * ch;
        if (int rc = segk_ws_grow(ctx, &ctx->fbt_tok, &ctx->fbt_tok_n, need, (size_t)need * sizeof(int32_t), st)) return rc;
        int32_t *range = ctx->fbt_tok, *new_tok = range + 2, *n_new = new_tok + ch;
        hipLaunchKernelGGL(k_fbi_predict_view, dim3((unsigned)((ch + 255) / 256)), dim3(256), 0, st, range, new_tok, n_new, (int)ch);
        SEGK_LAUNCH_CHECK();
        const size_t lds = fbi_predict_fixed_bytes(c->D, KM, true);
        for (int64_t r0 = 0; r0 < M; r0 += ch) {
            const int64_t n = M - r0 < ch ? M - r0 : ch;
            const segk_corpus v = fbi_query_view(c, Xq, ldq, r0, n);
            segk_fbatch btv = *bt;                          // one cell: the rows of the view (those beyond n_emb are left alone)
            btv.n_slices = btv.n_blocks = 1;
            btv.utt_range = btv.row_range = range;
            btv.prior_rows = prior_rows_q + r0;
            const int32_t n_utts[1] = {(int32_t)n};
            const double *fc_ll = nullptr;
            int ucap = 0;
            if (int rc = segk_fcb_token_ll(ctx, &v, f, &btv, 0, 1, 0, n_utts, new_tok, n_new, &fc_ll, &ucap, stream)) return rc;
            const unsigned grid = (unsigned)((n + FBI_T - 1) / FBI_T);
            if (c->x_dtype == SEGK_F32)
                hipLaunchKernelGGL((k_fbi_predict<float, 2>), dim3(grid), dim3(FBI_NT), lds, st, v, *f, *bt, r0, f->alpha,
                                   (const double *)prior_rows_q, (double *)nullptr, fc_ll, label, log_density, log_resp, resp_ld,
                                   probe_ll, probe_ld);
            else
                hipLaunchKernelGGL((k_fbi_predict<double, 2>), dim3(grid), dim3(FBI_NT), lds, st, v, *f, *bt, r0, f->alpha,
                                   (const double *)prior_rows_q, (double *)nullptr, fc_ll, label, log_density, log_resp, resp_ld,
                                   probe_ll, probe_ld);
            SEGK_LAUNCH_CHECK();
        }
        return SEGK_OK;
    }
    const int64_t n_tiles = (M + FBI_T - 1) / FBI_T;
    size_t lds;
    int per_launch;
    double *zbuf;
    if (int rc = fbi_predict_place(ctx, fbi_predict_fixed_bytes(c->D, KM, false), (size_t)FBI_T * KM * sizeof(double), (int)n_tiles, &lds,
                                   &per_launch, &zbuf, st))
        return rc;
#define SEGK_FBI_PREDICT(XT, COV)                                                                                               \
    do {                                                                                                                        \
        SEGK_CHECK_HIP(segk_dyn_lds((const void *)k_fbi_predict<XT, COV>, lds));                                                \
        for (int64_t t0 = 0; t0 < n_tiles; t0 += per_launch) {                                                                  \
            const int64_t r0 = t0 * FBI_T, n = M - r0 < (int64_t)per_launch * FBI_T ? M - r0 : (int64_t)per_launch * FBI_T;     \
            const segk_corpus v = fbi_query_view(c, Xq, ldq, r0, n);                                                            \
            hipLaunchKernelGGL((k_fbi_predict<XT, COV>), dim3((unsigned)((n + FBI_T - 1) / FBI_T)), dim3(FBI_NT), lds, st, v, *f, \
                               *bt, r0, f->alpha, (const double *)prior_rows_q, zbuf, (const double *)nullptr, label,           \
                               log_density, log_resp, resp_ld, probe_ll, probe_ld);                                             \
        }                                                                                                                       \
    } while (0)
    if (c->x_dtype == SEGK_F32) {
        if (f->cov_type == 0) SEGK_FBI_PREDICT(float, 0);
        else SEGK_FBI_PREDICT(float, 1);
    } else {
        if (f->cov_type == 0) SEGK_FBI_PREDICT(double, 0);
        else SEGK_FBI_PREDICT(double, 1);
    }
#undef SEGK_FBI_PREDICT
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

int32_t segk_fbi_predict_diag32(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, const void *Xq,
                                int64_t ldq, int64_t M, double *prior_rows_q, int32_t *label, double *log_density,
                                double *log_resp, int64_t resp_ld, double *probe_ll, int64_t probe_ld, void *stream)
{
    SEGK_REQUIRE(ctx && c && f && bt, "NULL argument");
    if (f->cov_type != 1) {
        segk_set_error("segk_fbi_predict_diag32: the float32 item likelihoods exist for diagonal components (cov_type 1) only, got "
                       "cov_type %d (fixed-variance and full-covariance components go through segk_fbi_predict)", (int)f->cov_type);
        return SEGK_ERR_UNSUPPORTED;
    }
    bool done;
    if (int rc = fbi_predict_check(ctx, c, f, bt, Xq, ldq, M, prior_rows_q, log_resp, resp_ld, probe_ll, probe_ld,
                                   "segk_fbi_predict_diag32", &done))
        return rc;
    SEGK_REQUIRE(bt->tab32 && bt->centre, "the float32 item likelihoods need segk_fbatch.tab32 (written by segk_fbb_prepare) and .centre");
    if (done) return SEGK_OK;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = fbi_predict_prior_rows(c, f, Xq, ldq, M, prior_rows_q, stream)) return rc;
    const int KM = f->K_max;
    const int64_t n_tiles = (M + FBI_T - 1) / FBI_T;
    size_t lds;
    int per_launch;
    double *zbuf;
    if (int rc = fbi_predict_place(ctx, fbi32_predict_fixed_bytes(c->D, KM), (size_t)FBI_T * fbi32_ldl(KM) * sizeof(double), (int)n_tiles,
                                   &lds, &per_launch, &zbuf, st))
        return rc;
#define SEGK_FBI32_PREDICT(XT)                                                                                                  \
    do {                                                                                                                        \
        SEGK_CHECK_HIP(segk_dyn_lds((const void *)k_fbi_predict_diag32<XT>, lds));                                              \
        for (int64_t t0 = 0; t0 < n_tiles; t0 += per_launch) {                                                                  \
            const int64_t r0 = t0 * FBI_T, n = M - r0 < (int64_t)per_launch * FBI_T ? M - r0 : (int64_t)per_launch * FBI_T;     \
            const segk_corpus v = fbi_query_view(c, Xq, ldq, r0, n);                                                            \
            hipLaunchKernelGGL(k_fbi_predict_diag32<XT>, dim3((unsigned)((n + FBI_T - 1) / FBI_T)), dim3(FBI32_NT), lds, st, v,  \
                               *f, *bt, r0, f->alpha, (const double *)prior_rows_q, zbuf, label, log_density, log_resp, resp_ld, \
                               probe_ll, probe_ld);                                                                             \
        }                                                                                                                       \
    } while (0)
    if (c->x_dtype == SEGK_F32) SEGK_FBI32_PREDICT(float);
    else SEGK_FBI32_PREDICT(double);
#undef SEGK_FBI32_PREDICT
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

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
    SEGK_REQUIRE(!c->vec_ids && !c->band_ids && c->N_max == 1 && c->n_utt == c->n_emb,
                 "a corpus of items: one one-landmark utterance per row, no span tables");
    if (int rc = fbi_check(c, f, bt, s_lo, s_n, b, probe_ll, probe_ld, "segk_fbi_assign")) return rc;
    FbbMap m;
    int most = 0;
    if (int rc = fbi_item_map(n_items, s_lo, s_n, &m, &most)) return rc;
    if (m.off[s_n] == 0) return SEGK_OK;
    return fbi_launch(ctx, c, f, bt, m, s_lo, s_n, b, n_items, most, sweep, anneal_temp, consider_unassigned, new_tok, n_new, probe_ll,
                      probe_ld, nullptr, stream);
}

int32_t segk_fbi_assign_diag32(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, int32_t s_lo,
                               int32_t s_n, int32_t b, const int32_t *n_items, uint64_t sweep, double anneal_temp,
                               int32_t consider_unassigned, const int32_t *new_tok, int32_t *n_new, double *probe_ll,
                               int64_t probe_ld, void *stream)
{
    SEGK_REQUIRE(ctx && c && f && bt && n_items && new_tok && n_new, "NULL argument");
    if (f->cov_type != 1) {
        segk_set_error("segk_fbi_assign_diag32: the float32 item step exists for diagonal components (cov_type 1) only, got "
                       "cov_type %d (fixed-variance and full-covariance components go through segk_fbi_assign)", (int)f->cov_type);
        return SEGK_ERR_UNSUPPORTED;
    }
    if (f->lm_unigram) {
        segk_set_error("segk_fbi_assign_diag32: the stand-alone batch sweep takes no language model");
        return SEGK_ERR_UNSUPPORTED;
    }
    SEGK_REQUIRE(bt->tab32 && bt->centre && bt->prior_rows,
                 "the float32 item step needs segk_fbatch.tab32 (written by segk_fbb_prepare), .centre and .prior_rows");
    SEGK_REQUIRE(!c->vec_ids && !c->band_ids && c->N_max == 1 && c->n_utt == c->n_emb,
                 "a corpus of items: one one-landmark utterance per row, no span tables");
    if (int rc = fbi_check(c, f, bt, s_lo, s_n, b, probe_ll, probe_ld, "segk_fbi_assign_diag32")) return rc;
    FbbMap m;
    int most = 0;
    if (int rc = fbi_item_map(n_items, s_lo, s_n, &m, &most)) return rc;
    if (m.off[s_n] == 0) return SEGK_OK;
    return fbi32_launch(ctx, c, f, bt, m, s_n, b, sweep, anneal_temp, consider_unassigned, n_new, probe_ll, probe_ld, nullptr, stream);
}

// The item half of a step of a MAP sweep (FBGMM.map_assign(sync="batch"); fbgmm.py:465-494 on slots, in place of the draws of
// fbgmm.py:436-460): segk_fbi_assign's checks, map and launches with the MAP half.
int32_t segk_fbi_assign_map(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, int32_t s_lo,
                            int32_t s_n, int32_t b, const int32_t *n_items, uint64_t sweep, int32_t consider_unassigned,
                            const int32_t *new_tok, int32_t *n_new, double *probe_ll, int64_t probe_ld, int32_t *n_moved,
                            void *stream)
{
    SEGK_REQUIRE(ctx && c && f && bt && n_items && new_tok && n_new && n_moved, "NULL argument");
    if (f->lm_unigram) {
        segk_set_error("segk_fbi_assign_map: the stand-alone batch sweep takes no language model");
        return SEGK_ERR_UNSUPPORTED;
    }
    SEGK_REQUIRE(!c->vec_ids && !c->band_ids && c->N_max == 1 && c->n_utt == c->n_emb,
                 "a corpus of items: one one-landmark utterance per row, no span tables");
    if (int rc = fbi_check(c, f, bt, s_lo, s_n, b, probe_ll, probe_ld, "segk_fbi_assign_map")) return rc;
    FbbMap m;
    int most = 0;
    if (int rc = fbi_item_map(n_items, s_lo, s_n, &m, &most)) return rc;
    if (m.off[s_n] == 0) return SEGK_OK;
    return fbi_launch(ctx, c, f, bt, m, s_lo, s_n, b, n_items, most, sweep, 1.0, consider_unassigned, new_tok, n_new, probe_ll, probe_ld,
                      nullptr, stream, n_moved);
}

int32_t segk_fbi_assign_map_diag32(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, int32_t s_lo,
                                   int32_t s_n, int32_t b, const int32_t *n_items, uint64_t sweep, int32_t consider_unassigned,
                                   const int32_t *new_tok, int32_t *n_new, double *probe_ll, int64_t probe_ld, int32_t *n_moved,
                                   void *stream)
{
    SEGK_REQUIRE(ctx && c && f && bt && n_items && new_tok && n_new && n_moved, "NULL argument");
    if (f->cov_type != 1) {
        segk_set_error("segk_fbi_assign_map_diag32: the float32 item step exists for diagonal components (cov_type 1) only, got "
                       "cov_type %d (fixed-variance and full-covariance components go through segk_fbi_assign_map)", (int)f->cov_type);
        return SEGK_ERR_UNSUPPORTED;
    }
    if (f->lm_unigram) {
        segk_set_error("segk_fbi_assign_map_diag32: the stand-alone batch sweep takes no language model");
        return SEGK_ERR_UNSUPPORTED;
    }
    SEGK_REQUIRE(bt->tab32 && bt->centre && bt->prior_rows,
                 "the float32 item step needs segk_fbatch.tab32 (written by segk_fbb_prepare), .centre and .prior_rows");
    SEGK_REQUIRE(!c->vec_ids && !c->band_ids && c->N_max == 1 && c->n_utt == c->n_emb,
                 "a corpus of items: one one-landmark utterance per row, no span tables");
    if (int rc = fbi_check(c, f, bt, s_lo, s_n, b, probe_ll, probe_ld, "segk_fbi_assign_map_diag32")) return rc;
    FbbMap m;
    int most = 0;
    if (int rc = fbi_item_map(n_items, s_lo, s_n, &m, &most)) return rc;
    if (m.off[s_n] == 0) return SEGK_OK;
    return fbi32_launch_form(ctx, c, f, bt, m, s_n, b, sweep, 1.0, consider_unassigned, n_new, probe_ll, probe_ld, nullptr, stream,
                             n_moved);
}

int32_t segk_fbi_assign_orphans(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, int32_t s_lo,
                                int32_t s_n, int32_t b, const int32_t *n_items, uint64_t sweep, const int32_t *was,
                                const int32_t *new_tok, int32_t *n_new, double *probe_ll, int64_t probe_ld, void *stream)
{
    SEGK_REQUIRE(ctx && c && f && bt && n_items && was && new_tok && n_new, "NULL argument");
    if (f->lm_unigram) {
        segk_set_error("segk_fbi_assign_orphans: the stand-alone mixture model takes no language model");
        return SEGK_ERR_UNSUPPORTED;
    }
    SEGK_REQUIRE(!c->vec_ids && !c->band_ids && c->N_max == 1 && c->n_utt == c->n_emb,
                 "a corpus of items: one one-landmark utterance per row, no span tables");
    if (int rc = fbi_check(c, f, bt, s_lo, s_n, b, probe_ll, probe_ld, "segk_fbi_assign_orphans")) return rc;
    // the cell's items bound its orphans: the lists and the grid are sized from them, a tile beyond the count returns at once
    FbbMap m;
    FbtList L = {};
    if (int rc = fbt_lists(ctx, c, bt, s_lo, s_n, b, n_items, n_items, new_tok, n_new, &m, &L, stream, was)) return rc;
    if (m.off[s_n] == 0) return SEGK_OK;
    return fbi_launch(ctx, c, f, bt, m, s_lo, s_n, b, n_items, 0, sweep, 1.0, 0, new_tok, n_new, probe_ll, probe_ld, &L, stream);
}

int32_t segk_fbt_assign(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, int32_t s_lo,
                        int32_t s_n, int32_t b, const int32_t *n_utts, const int32_t *tok_cap, uint64_t sweep, double anneal_temp,
                        const int32_t *new_tok, const int32_t *n_new, double *probe_ll, int64_t probe_ld, void *stream)
{
    SEGK_REQUIRE(ctx && c && f && bt && n_utts && tok_cap && new_tok && n_new, "NULL argument");
    if (f->lm_unigram) {
        segk_set_error("segk_fbt_assign: the acoustic-model batch sweep takes no language model (the bigram segmenter has no inner "
                       "sweeps: its reference asserts at am_n_iter > 0)");
        return SEGK_ERR_UNSUPPORTED;
    }
    SEGK_REQUIRE((c->vec_ids || c->band_ids) && c->n_utt > 0 && c->N_max > 0,
                 "a segmenter's corpus: utterances with span tables (the items of a stand-alone model go through segk_fbi_assign)");
    if (int rc = fbi_check(c, f, bt, s_lo, s_n, b, probe_ll, probe_ld, "segk_fbt_assign")) return rc;
    FbbMap m;
    FbtList L = {};
    if (int rc = fbt_lists(ctx, c, bt, s_lo, s_n, b, n_utts, tok_cap, new_tok, const_cast<int32_t *>(n_new), &m, &L, stream)) return rc;
    if (m.off[s_n] == 0) return SEGK_OK;
    return fbi_launch(ctx, c, f, bt, m, s_lo, s_n, b, n_utts, 0, sweep, anneal_temp, 0, new_tok, const_cast<int32_t *>(n_new), probe_ll,
                      probe_ld, &L, stream);
}

int32_t segk_fbt_assign_diag32(segk_ctx *ctx, const segk_corpus *c, const segk_fbgmm *f, const segk_fbatch *bt, int32_t s_lo,
                               int32_t s_n, int32_t b, const int32_t *n_utts, const int32_t *tok_cap, uint64_t sweep,
                               double anneal_temp, const int32_t *new_tok, const int32_t *n_new, double *probe_ll, int64_t probe_ld,
                               void *stream)
{
    SEGK_REQUIRE(ctx && c && f && bt && n_utts && tok_cap && new_tok && n_new, "NULL argument");
    if (f->cov_type != 1) {
        segk_set_error("segk_fbt_assign_diag32: the float32 token step exists for diagonal components (cov_type 1) only, got "
                       "cov_type %d (fixed-variance and full-covariance components go through segk_fbt_assign)", (int)f->cov_type);
        return SEGK_ERR_UNSUPPORTED;
    }
    if (f->lm_unigram) {
        segk_set_error("segk_fbt_assign_diag32: the acoustic-model batch sweep takes no language model (the bigram segmenter has "
                       "no inner sweeps: its reference asserts at am_n_iter > 0)");
        return SEGK_ERR_UNSUPPORTED;
    }
    SEGK_REQUIRE(bt->tab32 && bt->centre && bt->prior_rows,
                 "the float32 token step needs segk_fbatch.tab32 (written by segk_fbb_prepare), .centre and .prior_rows");
    SEGK_REQUIRE((c->vec_ids || c->band_ids) && c->n_utt > 0 && c->N_max > 0,
                 "a segmenter's corpus: utterances with span tables (the items of a stand-alone model go through segk_fbi_assign_diag32)");
    if (int rc = fbi_check(c, f, bt, s_lo, s_n, b, probe_ll, probe_ld, "segk_fbt_assign_diag32")) return rc;
    FbbMap m;
    FbtList L = {};
    if (int rc = fbt_lists(ctx, c, bt, s_lo, s_n, b, n_utts, tok_cap, new_tok, const_cast<int32_t *>(n_new), &m, &L, stream)) return rc;
    if (m.off[s_n] == 0) return SEGK_OK;
    return fbi32_launch(ctx, c, f, bt, m, s_n, b, sweep, anneal_temp, 0, const_cast<int32_t *>(n_new), probe_ll, probe_ld, &L, stream);
}

}  // extern "C"
