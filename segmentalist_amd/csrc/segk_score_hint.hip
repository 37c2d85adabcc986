// segk_score_hint.hip -- A1 with a HINT per row: the dense one-product fp16 contraction with a value-only top-2 drain, the
// hinted component scored in the reference's arithmetic beside it, and a certificate that verifies the hint against both.
// (one of the translation units of the k-means path; shared helpers: segk_kmeans_dev.h)
//
// KMeansComponents.argmax_neg_sqrd_norm_i (kmeans_components.py:225-232) is evaluated for every row in every sweep, and from
// one sweep to the next almost every row keeps its component (measured on the headline corpus: 6-17 % of the rows change
// in sweeps 2-10, 0.1 % once the chain has settled; tools/diag_hint_stability.py).  The one-product pre-filter
// (segk_score_h1.hip) spends as many vector-ALU issue cycles on its running top-2 -- five operations per two values, two
// of them only to remember WHICH pair won -- as its matrix pipe spends on the products, and pays a staging barrier per
// tile: 41 % matrix-pipe occupancy.  With a hint the index does not have to be tracked at all:
//
//   K1  k_kmeans_top2_rs   matrix waves: every (row, component) product on the matrix cores exactly as before (all K_max
//       slots, nothing skipped), but the drain keeps only the two largest VALUES per row: m1' = max3(m1, a, b),
//       m2' = max(m2, med3(m1, a, b)) -- three operations per two values.  Range-stationary: a workgroup (one per CU) copies
//       the fp16 tile images of ONE range of components into LDS once (16 tiles = 114 KB for the headline model) and its
//       matrix waves stream row blocks past them without a single barrier; the constants -|m|^2/2 enter as the C operand of
//       each block's first MFMA.  Output: (m1, m2) per (row, range).
//       hint waves (hint_wave_rows): for each row the hinted component h is scored in the reference's arithmetic,
//       s = -|x - m_h|^2; with -|x|^2 in the same summation order (nxx), f_h = (s + |x|^2) / 2 = x.m_h - |m_h|^2/2 is known
//       to within the reference's own rounding.  Output: {s, f_h, h} per row.
//   K2  k_hint_merge   the certificate, one thread per row.  With F the filter values (|F_k - f_k| <= E for every k),
//       top1 >= top2 their two largest (merged over the ranges) and tau >= 2 E + E2 the pre-filter's margin (filter_tau_h1):
//           top1 - top2 > tau            =>  the filter's argmax k1 is the reference's argmax      (as in the pre-filter)
//           f_h >= top1 - tau + E + dl   =>  h = k1: any other k has F_k <= top2, so f_k <= top2 + E < top1 - tau + E
//       (dl bounds the error of the computed f_h).  Both hold -> cand.k = h, cand.s = s: the reference's bits.  Otherwise
//       the row is queued for the second stage (the band stage, segk_score_band.hip; tables beyond its reach:
//       k_kmeans_score_sp, all three products) and, from there, the full scan -- exactly the rows the pre-filter would have
//       queued plus the rows whose hint was wrong.  A hint that names a component the filters' images carry as "absent" (an
//       exact duplicate of a lower row, segk_kmeans_mark_duplicates) is no hint: its F is not a bound on anything.
//
//       The certificate holds on a SUPERSET of the filter values (the delta score pass rests on this).  Let S' be any multiset
//       that contains F_h and, for every other current column k, a value >= F_k, and top1' >= top2' its two largest.  Suppose
//           top1' - top2' > tau   and   f_h >= top1' - tau + E + dl.
//       Then F_h >= f_h - E - dl >= top1' - tau > top2': F_h is the single largest member of S', every other member is
//       <= top2', hence for every k != h: f_k <= F_k + E <= top2' + E < top1' - tau + E <= f_h - dl -- h is the reference's
//       argmax.  Extra members (stale values of columns that have changed since) can only make the certificate fail, never
//       pass wrongly.
//
//   Delta score pass (k_delta_prep, K1 in delta mode, k_hint_merge): while a call repeats on the same rows, (m1, m2) of
//       the last FULL launch stay as the base, K1 multiplies only the columns whose image differs from that launch's snapshot
//       (packed into leading tiles), and the merge certifies against base U delta, a superset as above.  See k_delta_prep.
//       K1 is ONE launch either way: it reads the mode word k_delta_prep left and takes the full or the delta parameter set
//       (HintArgs), with the larger of the two grids and LDS sizes.  The hint waves decide which positions take their score
//       over from the previous call for a chunk of steps per round trip, and score the others -- the rows of the means that
//       moved -- 32 at a time in dense bodies, whichever steps they come from (hint_wave_rows).
//
//   Carry-over of a row's winner across the unchanged means (k_hint_merge in delta mode).  The certificate above cannot decide
//       a near-tie row -- its runner-up sits in the base within tau, sweep after sweep -- and the band stage then finds the
//       same winner among the same unchanged means every time.  A different argument decides such a row without the base.
//       Take a hinted call on the same call tuple as the previous hinted call (ctx->delta_key), the relabelling the identity.
//       For a row x let (k*, s*) be the reference's result of the PREVIOUS call: the first maximum over all K_max rows of
//       `means` as they were then.  Let U be the rows of `means` whose float32 bits are unchanged since that call
//       (meanchg[k] == 0), C the others.
//         (a) For k in U the reference's score of x against k is bit for bit what it was: same row, same mean, same
//             arithmetic.  So if k* is in U, k* is still the first maximum over U (scores and indices are what they were),
//             and the current result is the first maximum over {k*} u C.
//         (b) Hence x keeps (k*, s*) if every c in C scores strictly below s* in the reference.  (Strictly: with a tie a
//             c < k* would take the first maximum.)
//       The merge kernel proves (b) for a row at position p with hint h when ALL of these hold:
//         1. Mode: the mode word has SEGK_DELTA_MODE and SEGK_DELTA_SKIP -- the state is valid for this tuple, the previous
//            hinted call was on it, the relabelling is the identity.  Nothing else switches the carry-over on or off.
//         2. h >= 0 and h == lab_last[p], the label THIS LIBRARY recorded for the position in the previous call (DeltaBuf):
//            the hint where a certificate passed -- then h was the reference's argmax of that call --, the band stage's winner
//            where k_band_exact decided the row, -1 otherwise (full scan: such a row takes the normal route).  cand.k is the
//            caller's to write, so the hint alone proves nothing about the previous call; lab_last is private.  With it
//            h = k*.  (lab_base is another thing -- the label the BASE pass certified, whose stale F_h the merge drops -- and
//            stays apart: that repair needs F_h to have been the single largest base value, which a band winner's is not.)
//         3. meanchg[h] == 0: k* is in U, and the hint waves' {s, f_h} for h -- recomputed, or taken over under the same
//            condition -- is s* itself and its filter-domain value.
//         4. Every c in C has its CURRENT filter value in the packed delta image: no k with meanchg[k] && !colchg[k].  (A
//            float32 mean can move below the resolution of the fp16 image: no image bit changes, nothing is packed, and the
//            base's top-2 say nothing about that column alone.)  Decided per call by every workgroup from the two flag arrays;
//            if it fails, no row is carried in this call.  Exempt: a column the current image marks "absent" -- an exact
//            duplicate of a lower row i.  Its score is i's bit for bit and its index is higher, so it is the first maximum of
//            no set that contains i; and i is in U (score <= s*, and i > k* where equal, or i = k*), or in C and bounded here,
//            or absent itself with a still lower original.
//         5. Margin: f_h > d1 * unscale + (e1 + rnd + dl) * 1.0001, d1 = the row's part_delta m1, the largest current filter
//            value over the packed columns (-inf: nothing packed).  With 4 every c in C that is not absent has F_c <= d1, and
//            this is the slack the certificate above leaves between any competitor's filter value and f_h
//            (top2 < top1 - tau <= f_h - (E + dl), E = e1 + rnd): f_c <= F_c + E < f_h - dl, so c loses to h in the
//            reference's arithmetic exactly as every k != h does there.  The bounds are those tests/test_filter_bounds_cpu.py
//            proves for the certificate; the carry-over adds none.  (A packed column that is h's own -- changed against the
//            base earlier, unchanged since the previous call -- makes d1 >= F_h: the test fails and the row takes the
//            normal route.  A changed mean bit-identical to h's has F_c = F_h: likewise.)
//       Then cand.k = h, cand.s = s, lab_last[p] = h, and the row is not queued.  A wrong or garbage hint fails 2 and costs
//       only time.  Every call that has delta state writes lab_last for every position, full mode included; a call without
//       (another table, an id list, a sub-range, an un-hinted call in between, a reallocation) clears delta_valid, the next
//       mode word has no SEGK_DELTA_SKIP, and lab_last is rewritten before it is read again.
//
// Results are those of segk_kmeans_score whatever the hints are (a wrong hint costs time, never correctness); the
// full-size parity tests run this path against the C oracle row by row.
#include "segk_kmeans_dev.h"

#define SEGK_K1_NW 4                 /* matrix waves per workgroup of K1, and as many hint waves */
#define SEGK_HINT_CHUNK 8            /* steps of 32 rows whose skip a hint wave decides in one round trip (delta score pass) */

// development, timing only (-DSEGK_K1_ABL=n, results wrong): 1 no drain in the tile loop, 2 no operand refill from LDS
#ifndef SEGK_K1_ABL
#define SEGK_K1_ABL 0
#endif

// What K1's matrix waves multiply and where the result goes.  A launch carries two sets, one for a full and one for a delta
// pass (one range over the packed image of the changed columns), and takes the one the mode word k_delta_prep left names.
struct K1Set {
    const float *tiles;             // first tile of the fp16x2 image the matrix waves multiply
    int n_tiles;                    // its tiles (delta set: at launch time unknown, read from ctl[2])
    int tpr, n_ranges;              // tiles per LDS range (the label map sits behind them in LDS), ranges
    float2 *part;                   // [n_ranges][n] (m1, m2) in the scaled domain of the images
    int grid;                       // workgroups; the launch has the larger of the two sets', and a workgroup beyond this one returns
};

struct HintArgs {
    const unsigned char *ximg;      // fp16x2 row image (segk_corpus.Xb3): header, then plane 0 [n_emb][KP]
    const int32_t *ids;
    int64_t row0, n;
    K1Set full, delta;              // full: the model's whole image (tiles_b3 + 1024; also the "absent" marks of the label map);
                                    // delta: the packed image, unused without `ctl`
    int K_max;
    // development (SEGK_HINT_DBG, results wrong; bits): 1 no result stores, 4 the first rows loaded behind the LDS fill, 8 no hint
    // waves, 16 their rows from a cache-resident corner, 32 one block of their arithmetic, 64 paced, 128 no matrix waves
    int dbg;
    unsigned long long *stamp;      // development (-DSEGK_STAMP builds): per wave {cycles in the row waits, in the tile loops, total, groups}
    float *fb_w;                    // [3][8] share of the row groups each XCD took in the launches L - 1, L, L + 1 (slot = launch % 3)
    unsigned int *fb_t;             // [3][8] how long its waves lived (s_memrealtime ticks, maximum); NULL: equal shares
    int fb_cur;                     // this launch's slot
    const int32_t *remap;           // previous label -> current label (NULL: identity)
    int32_t *zero_cnt, *pre_hdr;    // the caller's ambiguity-queue length (may be NULL) and the undecided-row queue's header [16]: cleared here
    int64_t k1_groups;              // groups this kernel multiplies (the few behind the last whole round of all waves go to the full scan)
    // the hint waves (waves 4 .. 7 of every workgroup): the hinted component of every row scored in reference arithmetic
    const float *xrows32;           // float32 rows [n_emb][ld32]
    int64_t ld32;
    const float *means32;           // float32 `means` [K_max][D]
    const int32_t *cand_k;          // per row: the label the previous call left (the hint, in that call's labelling)
    const float *nxx;               // -|x|^2 per row in the reference's summation order (k_corpus_resid_sp)
    float4 *hint_out;               // [n] by position in the launch: {s = -|x - m_h|^2, f_h = x.m_h - |m_h|^2/2, bits of h (-1: no hint), 0}
    // delta score pass (NULL: none, the full set): the control words k_delta_prep left and the rows of `means` whose bits changed
    // since the previous call
    int32_t *ctl;
    const int32_t *meanchg;
    float *snap_img;                // the base pass's image, refreshed by the full launch: [4 floats: exponent][n_tiles][KS * 256 + 32]
};

// ---- delta score pass: state and control ----------------------------------------------------------------------------------
// ctl[0] mode word (SEGK_DELTA_*), [1] columns of the image that differ from the base pass's snapshot, [2] tiles of the packed
// delta image (0 in full mode), [3] positions the hint waves skipped (cleared by k_delta_prep, added to by K1), [4] packed tiles
// multiplied since the base pass, [5 + parity] rows of `means` that changed during the call of that parity, [7] ctl[1] of the
// previous call, [8] the number of active components at the previous call, [12..15] and [18] what a prep found in [5 + other
// parity], [4], [7], [8] and in the snapshot's exponent (for a prep that repeats it), [16..17] a 64-bit word: the prep's
// changed-column count, tickets and relabelled tiles (delta_prep_tile, segk_kmeans_dev.h; zero between launches)
#define SEGK_MEANCHG_BIT 0x40000000  /* in the hint waves' label map: the float32 mean of this component changed since the previous call */

// ---- K1 ---------------------------------------------------------------------------------------------------------------
// SEGK_K1_NW = 4 matrix waves per workgroup (and as many hint waves), one workgroup per CU: ONE matrix wave per SIMD -- the
// rows of the wave's next group are prefetched into a second register set while the current group is multiplied, and
// nothing but the wave's own instruction stream decides whether the matrix pipe idles: per 32-cycle MFMA slot the MFMA's
// issue (8 cycles) and 3-4 vector operations of the other block's drain.  (Two matrix waves per SIMD without prefetch fill
// each other's gaps at group boundaries but compete for the SIMD's vector issue inside the tile loop: 6 % slower, retired.)
//
// Drain of a block's 16 values per lane, four at a time, value-only (no index): with x1 = max3(m1, a, b),
// t1 = med3(m1, a, b) [the second largest of m1, a, b], u = med3(x1, c, d) [the second largest of x1, c, d]:
//     m1' = max3(x1, c, d)     m2' = max3(m2, t1, u)
// (the second largest of {m1, a, b, c, d} is max(t1, u): t1 <= x1, and whichever of x1, c, d is largest, u is the runner-up
// among them) -- five operations per four values.  Operation 0 of a quad is a compiler-visible builtin, so that the hazard
// recogniser sees the first read of the MFMA's result; the others are single-instruction asm (fmaxf() would add a
// canonicalising v_max per MFMA output, and the scheduler may not reorder asm volatile).
// One quad = one asm block (the compiler pads every asm statement that a vector instruction of its own follows with an
// s_nop 0, four cycles of issue each: with one statement per operation the nops were a fifth of the loop's issue slots, and a
// lone wave has none to spare).  FIRST: the quad that opens a block's drain -- its first operation, the first read of the
// MFMA's result, stays a compiler-visible builtin so that the hazard recogniser places the wait states the matrix pipe needs.
#define SEGK_RS_DRAIN_QUAD(O_, AO, q_, FIRST)                                                                               \
    do {                                                                                                                     \
        float x1_, u_;                                                                                                       \
        if (FIRST) {                                                                                                         \
            const float t1_ = __builtin_amdgcn_fmed3f(m1[O_], AO[4 * (q_)], AO[4 * (q_) + 1]);                              \
            asm volatile("v_max3_f32 %2, %0, %4, %5\n\t"                                                                     \
                         "v_med3_f32 %3, %2, %6, %7\n\t"                                                                     \
                         "v_max3_f32 %0, %2, %6, %7\n\t"                                                                     \
                         "v_max3_f32 %1, %1, %8, %3"                                                                          \
                         : "+v"(m1[O_]), "+v"(m2[O_]), "=&v"(x1_), "=&v"(u_)                                                 \
                         : "v"(AO[4 * (q_)]), "v"(AO[4 * (q_) + 1]), "v"(AO[4 * (q_) + 2]), "v"(AO[4 * (q_) + 3]), "v"(t1_)); \
        } else {                                                                                                             \
            float t1_;                                                                                                       \
            asm volatile("v_med3_f32 %4, %0, %5, %6\n\t"                                                                     \
                         "v_max3_f32 %2, %0, %5, %6\n\t"                                                                     \
                         "v_med3_f32 %3, %2, %7, %8\n\t"                                                                     \
                         "v_max3_f32 %0, %2, %7, %8\n\t"                                                                     \
                         "v_max3_f32 %1, %1, %4, %3"                                                                          \
                         : "+v"(m1[O_]), "+v"(m2[O_]), "=&v"(x1_), "=&v"(u_), "=&v"(t1_)                                     \
                         : "v"(AO[4 * (q_)]), "v"(AO[4 * (q_) + 1]), "v"(AO[4 * (q_) + 2]), "v"(AO[4 * (q_) + 3]));         \
        }                                                                                                                    \
    } while (0)

// ---- the hint waves of K1 -----------------------------------------------------------------------------------------------
// K1's four matrix waves leave the chip's memory system nearly idle (224 bytes per row and 200 us: 1.2 TB/s) and every SIMD a
// second wave slot.  Four more waves per workgroup use both: they stream the float32 rows ONCE, contiguously (whole 128-byte
// lines: a step is 32 consecutive rows), fetch each row's hinted component from the float32 table (400 KB: L2-resident) and
// evaluate the reference's -|x - m_h|^2 in numpy's pairwise order -- TWO lanes per row (h = 0, 1: the lane halves of the eight
// strided accumulators), packed fp32 arithmetic with every half rounded like the scalar operation.  Nothing here depends on the
// matrix waves' results: the certificate (top-2 of ALL ranges against f_h) is taken afterwards by k_hint_merge, one pass over
// 48 bytes per row.  Round 3 did this as a kernel of its own behind K1 (k_kmeans_hint_exact: 129 us, 572 MB fetched because
// its range workgroups picked scattered rows); fused, the float32 corpus crosses HBM once per sweep, under the matrix work.
template <int KS, int V>
__device__ __forceinline__ void hint_wave_rows(const HintArgs &H, const int32_t *map /* LDS */, int64_t w, int64_t n_w, bool skip_ok)
{
    constexpr int D = 16 * KS - 4 * V;
    constexpr int nfull = D & ~7, nblk = nfull >> 3, rem = D & 7;
    constexpr int NX = nblk + (rem ? 1 : 0);
    typedef float f32x4_t __attribute__((ext_vector_type(4)));
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    typedef const __attribute__((address_space(1))) f32x4_t *gptr_t;
    const int lane = threadIdx.x & 63, row = lane >> 1, h = lane & 1;
    auto pk_sub = [](f32x2_t a, f32x2_t b2) -> f32x2_t {           // a - b, both halves in one instruction
        f32x2_t d;
        asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b2));
        return d;
    };
    const int64_t n_steps = (H.n + 31) >> 5;
    if (H.dbg & 8) return;                                         // development (make DEV=1): timing without the hint waves' work
    auto rid_of = [&](int64_t s_) -> int32_t {
        const int64_t p_ = s_ * 32 + row;
        return p_ < H.n ? (H.ids ? H.ids[p_] : (int32_t)(H.row0 + p_)) : -1;
    };
    // one body: 32 positions, one per lane pair.  The hinted component `hint` (-1: none) of row rid_c (-1: no row) scored and
    // stored at position p unless `skip`; position, row and hint are the lane's own (a step of 32 consecutive rows in the serial
    // loop, 32 entries of the pending list in the delta score pass).  `mid` runs between the body's loads and its arithmetic
    // (the serial loop's prefetch of the next step)
    auto step_body = [&](int64_t p, int32_t rid_c, int32_t hint, bool skip, auto &&mid) {
        f32x4_t xv[NX], mv[NX];
#pragma unroll
        for (int b = 0; b < NX; b++) { xv[b] = f32x4_t{0.f, 0.f, 0.f, 0.f}; mv[b] = xv[b]; }
        if (!skip) {
            int64_t r_any = rid_c >= 0 ? (int64_t)rid_c : (H.ids ? 0 : H.row0);
            if (H.dbg & 16) r_any &= 1023;                          // development: the rows from a cache-resident corner (timing)
            const uintptr_t xa = (uintptr_t)(H.xrows32 + r_any * H.ld32);
            const uintptr_t ma = (uintptr_t)(H.means32 + (int64_t)(hint >= 0 ? hint : 0) * D);
#pragma unroll
            for (int b = 0; b < nblk; b++) xv[b] = *reinterpret_cast<gptr_t>(xa + 16u * h + 32u * b);
            if constexpr (rem != 0) xv[nblk] = *reinterpret_cast<gptr_t>(xa + 4u * nfull);
#pragma unroll
            for (int b = 0; b < nblk; b++) mv[b] = *reinterpret_cast<gptr_t>(ma + 16u * h + 32u * b);
            if constexpr (rem != 0) mv[nblk] = *reinterpret_cast<gptr_t>(ma + 4u * nfull);
        }
        const float nx = rid_c >= 0 ? H.nxx[rid_c] : 0.f;
        if (H.dbg & 64) __builtin_amdgcn_s_sleep(64);               // development: paced hint waves
        mid();
        // the reference's float32 -(deltas*deltas).sum() in numpy's pairwise order: this lane owns the strided accumulators
        // r_{4h..4h+3}
        f32x2_t rl = {0.f, 0.f}, rh = {0.f, 0.f};
#pragma unroll
        for (int b = 0; b < ((H.dbg & 32) ? 1 : nblk); b++) {      // (dbg 32, development: one block of the arithmetic only)
            const f32x2_t dl = pk_sub(mv[b].xy, xv[b].xy), dh = pk_sub(mv[b].zw, xv[b].zw);
            const f32x2_t tl = dl * dl, th = dh * dh;
            rl = b == 0 ? tl : rl + tl;
            rh = b == 0 ? th : rh + th;
        }
        float res = (rl.x + rl.y) + (rh.x + rh.y);
        const float ro = __shfl_xor(res, 1);
        res = (h == 0) ? res + ro : ro + res;                      // ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7))
        if constexpr (rem != 0) {
            const f32x2_t dl = pk_sub(mv[nblk].xy, xv[nblk].xy), dh = pk_sub(mv[nblk].zw, xv[nblk].zw);
            const f32x2_t tl = dl * dl, th = dh * dh;
            res += tl.x;
            if (rem > 1) res += tl.y;
            if (rem > 2) res += th.x;
            if (rem > 3) res += th.y;
        }
        const float sc = -res;                                     // -|x - m_h|^2
        if (h == 0 && p < H.n && !skip) H.hint_out[p] = make_float4(sc, 0.5f * (sc - nx), __int_as_float(rid_c >= 0 ? hint : -1), 0.f);
    };
    int n_skipped = 0;
    if (skip_ok) {
        // delta score pass.  Where the component the previous call scored for a position (its hint_out entry) is the current hint
        // and that mean's bits have not changed, the entry IS this call's result: same row, same mean, same arithmetic -- no row,
        // no mean, no store.  Once the chain has settled that is nearly every position, and a step that waits for its labels
        // only to find nothing to do is a bare round trip (32 of them in a row per wave on the headline corpus).  So the test is
        // taken for a CHUNK of the wave's steps at once, one lane per position and SEGK_HINT_CHUNK / 2 positions per lane, all
        // its loads in flight together.
        //
        // Dense bodies.  The positions that are NOT skipped (the live ones) are the rows of the means that moved, scattered over
        // the corpus: with 5 % of them live, four steps in five have one or two, and a body per such step is a dependent round
        // trip with one or two of its 32 row slots in use.  So the live positions of a chunk go onto a pending list in a fixed
        // order (step by step, row by row: the chunk's order), and a body runs whenever 32 are pending, and once more at the end
        // of the wave's steps.  The list is not stored anywhere: entry j of a chunk is the j-th set bit of the chunk's ballots,
        // a lane pair finds the lane that holds it (sel_bit) and pulls row and hint from it (ds_bpermute); the fewer than 32
        // entries left over at a chunk's end stay in the lane pairs' registers (c_*).  Registers, not LDS: the LDS behind the
        // label map is what the tile plan (segk_hint_plan) and the delta launch's tile cap are sized from, and a list there
        // (4 waves x 287 entries, 14 KB) would move both for every table -- this way no launch's plan changes.  The next chunk's
        // loads are issued in front of the current chunk's bodies, so the test's round trip is not between bodies.  (Two bodies
        // in flight -- the next body's rows loaded under this one's arithmetic -- would need a second row and mean set, 104 more
        // registers at D = 100: above the kernel's budget, left out.)  A position is written only by the wave that owns its step.
        constexpr int CH = SEGK_HINT_CHUNK, PPL = CH / 2;
        const int crow = lane & 31, chalf = lane >> 5;             // the test's lane: position crow of the chunk's step 2 u + chalf
        auto chunk_load = [&](int64_t s0, int32_t (&rd)[PPL], int32_t (&kp)[PPL], int32_t (&pzv)[PPL]) __attribute__((always_inline)) {
#pragma unroll
            for (int u = 0; u < PPL; u++) {
                const int64_t s_ = s0 + (int64_t)(2 * u + chalf) * n_w, p_ = s_ * 32 + crow;
                const bool in = s_ < n_steps && p_ < H.n;
                rd[u] = in ? (H.ids ? H.ids[p_] : (int32_t)(H.row0 + p_)) : -1;
                pzv[u] = in ? __float_as_int(H.hint_out[p_].z) : -2;
            }
#pragma unroll
            for (int u = 0; u < PPL; u++) kp[u] = rd[u] >= 0 ? H.cand_k[rd[u]] : -1;
        };
        // the n-th set bit (0 .. 31) of w_, n_ < popcount(w_) (anything in 0 .. 31 otherwise)
        auto sel_bit = [](unsigned w_, int n_) __attribute__((always_inline)) -> int {
            int base = 0;
#pragma unroll
            for (int sh = 16; sh >= 1; sh >>= 1) {
                const int t = __popc(w_ & ((1u << sh) - 1u));
                const bool up = n_ >= t;
                w_ = up ? w_ >> sh : w_;
                base += up ? sh : 0;
                n_ -= up ? t : 0;
            }
            return base & 31;
        };
        int c_n = 0;                                               // entries carried over from the chunks before: 0 .. 31
        int64_t c_p = 0;                                           // ... lane pair `row` holds entry `row`: position, row, hint
        int32_t c_rid = -1, c_hint = -1;
        int32_t rd_n[PPL], kp_n[PPL], pz_n[PPL];                   // the loads of the chunk ahead
        chunk_load(w, rd_n, kp_n, pz_n);
        for (int64_t s0 = w; s0 < n_steps; s0 += (int64_t)CH * n_w) {
            int32_t rd[PPL], hv[PPL];                              // per position of the chunk: row, hint
            unsigned long long live[PPL];
            int pre[PPL + 1];                                      // live positions in front of part u of the chunk
            pre[0] = 0;
#pragma unroll
            for (int u = 0; u < PPL; u++) {
                const int64_t s_ = s0 + (int64_t)(2 * u + chalf) * n_w;
                const bool in = s_ < n_steps && s_ * 32 + crow < H.n;
                rd[u] = rd_n[u];
                int32_t hint = (rd[u] >= 0 && kp_n[u] >= 0 && kp_n[u] < H.K_max) ? map[kp_n[u]] : -1;
                const bool mchg = hint >= 0 && (hint & SEGK_MEANCHG_BIT) != 0;
                if (hint >= 0) hint &= ~SEGK_MEANCHG_BIT;
                const bool skip = rd[u] >= 0 && hint >= 0 && !mchg && pz_n[u] == hint;
                hv[u] = hint;
                live[u] = __ballot(in && !skip);
                pre[u + 1] = pre[u] + __popcll(live[u]);
                n_skipped += __popcll(__ballot(skip));
            }
            const int64_t s1 = s0 + (int64_t)CH * n_w;
            chunk_load(s1, rd_n, kp_n, pz_n);                     // (beyond the last step: no load, every lane masks its own)
            if (pre[PPL] == 0) continue;                           // nothing new: the carried entries wait on
            const int total = c_n + pre[PPL];
            // entry g0 + row of the list (the carried entries, then the chunk's) for this lane pair; false: beyond the list
            // (step i of the chunk is word i of the ballots -- the low half of live[i / 2] for an even i, the high half for an odd
            // one -- and `at` the entries in front of it.  Every choice below is a chain of selects on thresholds of j_:
            // written as "the u-th of an array" the compiler puts the array into scratch and indexes it per lane.)
            auto fetch = [&](int g0, int64_t &p_e, int32_t &rid_e, int32_t &hint_e) __attribute__((always_inline)) -> bool {
                const int g_ = g0 + row, j_ = g_ - c_n;
                unsigned w_ = (unsigned)live[0];
                int i_ = 0, jj = j_;
#pragma unroll
                for (int i = 1; i < CH; i++) {
                    const int at = (i & 1) ? pre[i >> 1] + __popc((unsigned)live[i >> 1]) : pre[i >> 1];
                    const unsigned wi = (i & 1) ? (unsigned)(live[i >> 1] >> 32) : (unsigned)live[i >> 1];
                    const bool up = j_ >= at;
                    w_ = up ? wi : w_;
                    i_ = up ? i : i_;
                    jj = up ? j_ - at : jj;
                }
                const int src = 32 * (i_ & 1) + sel_bit(w_, jj);    // the test's lane that holds the entry
                int32_t r_ = __shfl(rd[0], src), h_ = __shfl(hv[0], src);
#pragma unroll
                for (int u = 1; u < PPL; u++) {
                    const int32_t ru = __shfl(rd[u], src), hu = __shfl(hv[u], src);
                    const bool up = j_ >= pre[u];
                    r_ = up ? ru : r_;
                    h_ = up ? hu : h_;
                }
                const int64_t s_ = s0 + (int64_t)i_ * n_w;
                const bool carried = j_ < 0;
                p_e = carried ? c_p : s_ * 32 + (src & 31);
                rid_e = carried ? c_rid : r_;
                hint_e = carried ? c_hint : (r_ >= 0 ? h_ : -1);
                return g_ < total;
            };
            int done = 0;
#pragma unroll 1
            for (; total - done >= 32; done += 32) {
                int64_t p_e;
                int32_t rid_e, hint_e;
                fetch(done, p_e, rid_e, hint_e);
                step_body(p_e, rid_e, hint_e, false, [] {});
            }
            {
                int64_t p_e;
                int32_t rid_e, hint_e;
                const bool on = fetch(done, p_e, rid_e, hint_e);
                c_p = p_e; c_rid = on ? rid_e : -1; c_hint = on ? hint_e : -1;
                c_n = total - done;
            }
        }
        if (c_n > 0) step_body(c_p, c_rid, c_hint, row >= c_n, [] {});
        if (n_skipped > 0 && lane == 0) atomicAdd(H.ctl + 3, n_skipped);
        return;
    }
    int64_t s = w;
    // row ids two steps ahead, previous labels one step ahead: no load of a step waits for another load of the same step
    int32_t rid = -1, rid_n = -1, kprev = -1;
    if (s < n_steps) {
        rid = rid_of(s);
        if (s + n_w < n_steps) rid_n = rid_of(s + n_w);
        kprev = rid >= 0 ? H.cand_k[rid] : -1;
    }
    for (; s < n_steps; s += n_w) {
        int32_t hint = (rid >= 0 && kprev >= 0 && kprev < H.K_max) ? map[kprev] : -1;
        if (hint >= 0) hint &= ~SEGK_MEANCHG_BIT;
        // the next step's previous labels and the row ids of the step after it travel under this step's arithmetic
        step_body(s * 32 + row, rid, hint, false, [&] {
            rid = rid_n;
            kprev = rid >= 0 ? H.cand_k[rid] : -1;
            const int64_t s2 = s + 2 * n_w;
            rid_n = s2 < n_steps ? rid_of(s2) : -1;
        });
    }
}

// ---- the XCDs' shares of K1's row groups ----------------------------------------------------------------------------------
// Under K1 the chip runs into its power limit, and the eight XCDs then hold DIFFERENT clocks (1.65-1.77 GHz measured, the same
// XCDs slow launch after launch): with equal shares the fast ones idle for the last 10-20 us of 200.  So an XCD takes a
// contiguous share of the groups in proportion to the rate it showed in the previous launch: its share then / the lifetime of
// its waves = the rate; new share = half the old one, half the rate's.  Nothing is exchanged during the launch, and the results
// do not depend on who computes which rows.  Every wave does the arithmetic for itself (one load round trip, sums and prefix by
// shuffles; lane x & 7 = XCD x) and gets the groups [lo, hi) of its workgroup's XCD; `record`: this wave leaves the shares for the
// next launch (a delta launch measures nothing: it hands the last full launch's shares and lifetimes on).
struct XcdShare { int64_t lo, hi; };
__device__ __forceinline__ XcdShare k1_xcd_share(const HintArgs &H, int64_t total_groups, bool delta, bool record)
{
    const int lane = threadIdx.x & 63, x = lane & 7;
    const int cur = H.fb_cur, prev = (cur + 2) % 3, next = (cur + 1) % 3;
    const float wp = H.fb_w[prev * 8 + x];
    const unsigned int tp = H.fb_t ? H.fb_t[prev * 8 + x] : 0u;
    const bool ok = __all(tp > 0u && wp > 0.f);
    const float rate = ok ? wp / (float)tp : 0.f;
    float rsum = rate;
    rsum += __shfl_xor(rsum, 1);
    rsum += __shfl_xor(rsum, 2);
    rsum += __shfl_xor(rsum, 4);
    float w = !(wp > 0.f) ? 0.125f : ok ? 0.5f * wp + 0.5f * (rate / rsum) : wp;
    w = fminf(fmaxf(w, 0.0625f), 0.25f);
    float wsum = w;
    wsum += __shfl_xor(wsum, 1);
    wsum += __shfl_xor(wsum, 2);
    wsum += __shfl_xor(wsum, 4);
    double cum = 0.0;                                        // exclusive prefix in XCD order, every lane the same additions
    for (int y = 0; y < 8; y++) {
        const float wy = __shfl(w, y);
        if (y < x) cum += (double)wy;
    }
    const int64_t split = (int64_t)(cum * ((double)total_groups / (double)wsum));
    const int xcd = blockIdx.x & 7;
    XcdShare s;
    s.lo = __shfl(split, xcd);
    s.hi = xcd == 7 ? total_groups : __shfl(split, (xcd + 1) & 7);
    if (record && lane < 8) {
        H.fb_w[cur * 8 + x] = delta ? (wp > 0.f ? wp : 0.125f) : w / wsum;
        if (H.fb_t) {
            H.fb_t[next * 8 + x] = 0u;
            if (delta) H.fb_t[cur * 8 + x] = tp;
        }
    }
    return s;
}

// (launch bounds "two waves per SIMD", a matrix and a hint wave: 256 registers per lane, all of them vector registers.  Given
// 512 the compiler keeps the accumulators in the accumulator file and copies every value out for the drain, 16 v_accvgpr_read
// per block)
template <int KS, int V>
__global__ __launch_bounds__(128 * SEGK_K1_NW, 1) void k_kmeans_top2_rs(HintArgs H)
{
    typedef _Float16 T;
    typedef SegkPiece::V8 V8;
    // (only 256 of a wave's registers are addressable by vector instructions: a second 4-block row set lands in the accumulator
    // file and is copied back and forth -- 5 000 v_accvgpr moves.  So: two blocks of 32 rows per group, the next group's prefetched)
    constexpr int P = 2, KP = KS * 16, NBLK = 2;
    constexpr int STRIDE = (KS * P * 256 + 32 + 1023) / 1024 * 1024;      // floats per tile of the global image
    constexpr int TL = KS * 256 + 32;                                     // floats per tile in LDS: KS piece-0 blocks + constants
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    // The mode word picks the parameter set (no control words: the full one).  Everything below that depends on the grid uses
    // the set's own (`grid`), never gridDim.x: the launch has the larger of the two.
    // (readfirstlane: the words are the same for every lane, and what follows from them -- the set's grid, pointers, tile and
    // group counts -- belongs in scalar registers, not in a copy per lane)
    const int mw = H.ctl ? __builtin_amdgcn_readfirstlane(H.ctl[0]) : 0;
    const bool delta = (mw & SEGK_DELTA_MODE) != 0, skip_ok = (mw & SEGK_DELTA_SKIP) != 0;
    const K1Set S = delta ? H.delta : H.full;
    // (delta mode: the tile count from device memory; none: no matrix work, the hint waves only)
    const int n_tiles = delta ? __builtin_amdgcn_readfirstlane(H.ctl[2]) : S.n_tiles;
    const int tpr = S.tpr, R = S.n_ranges, grid = S.grid;
    const float *tiles = S.tiles;
    float2 *part = S.part;
    if ((int)blockIdx.x >= grid) return;
    const int map_off = tpr * TL;                                         // floats: the label map behind the mode's tiles
    const bool is_hint = wave >= SEGK_K1_NW;                // waves SEGK_K1_NW .. 2 SEGK_K1_NW - 1: hint_wave_rows
    if (!is_hint) __builtin_amdgcn_s_setprio(2);    // the matrix waves first wherever the two kinds meet at an issue port
#ifdef SEGK_STAMP
    const unsigned long long st_k0 = __builtin_amdgcn_s_memtime(), st_r0 = __builtin_amdgcn_s_memrealtime();
#endif
    // workgroup -> (range, slot).  Workgroups b and b + 8 share an XCD (round-robin placement, speed only): the R
    // workgroups that stream the same rows sit on one XCD when the grid allows, so that the rows cross HBM once
    int range, wgr, n_wgr;
    const bool xcd_aware = (grid & 7) == 0 && ((grid >> 3) % R) == 0;
    if (xcd_aware) {
        const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
        range = idx % R;
        wgr = (idx / R) * 8 + xcd;
        n_wgr = grid / R;
    } else {
        n_wgr = grid / R;
        range = blockIdx.x % R;
        wgr = blockIdx.x / R;
    }
    const int t_lo = range * tpr;
    int nt = n_tiles - t_lo;
    if (nt > tpr) nt = tpr;
    // (a workgroup without matrix work -- beyond the last whole set of ranges, or a range without tiles -- still runs its hint waves)
    const bool mm_on = wgr < n_wgr && nt > 0;
    if (nt < 1) nt = 1;
    const T *plane0 = (const T *)(H.ximg + SEGK_SP_HEADER);
    // this wave's row groups: g_first, g_first + n_slots, ... below n_groups
    const int64_t total_groups = (H.n + 32 * NBLK - 1) / (32 * NBLK);
    int64_t n_groups = H.k1_groups < total_groups ? H.k1_groups : total_groups, n_slots = (int64_t)n_wgr * SEGK_K1_NW, g_first = (int64_t)wgr * SEGK_K1_NW + wave;
    const unsigned long long fb_t0 = __builtin_amdgcn_s_memrealtime();
    // the queue lengths of the call cleared: the caller's ambiguity queue (when segk_kmeans_score_hinted deferred it) and the
    // second stage's counters
    if (blockIdx.x == 0 && tid == 0) {
        if (H.zero_cnt) *H.zero_cnt = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) H.pre_hdr[i] = 0;
    }
    const XcdShare share = k1_xcd_share(H, total_groups, delta, blockIdx.x == 0 && wave == 0);
    const bool fb = xcd_aware && H.fb_t != nullptr && !delta;     // (a delta launch is not power-limited: equal shares)
    if (fb) {
        n_slots = (int64_t)(n_wgr >> 3) * SEGK_K1_NW;
        g_first = share.lo + (int64_t)(wgr >> 3) * SEGK_K1_NW + wave;
        n_groups = share.hi;
    }

    // the rows of group g into a register set
#define SEGK_RS_LOAD(g_, XB)                                                                                    \
    do {                                                                                                         \
        _Pragma("unroll") for (int b = 0; b < NBLK; b++) {                                                       \
            const int64_t r = (g_) * (32 * NBLK) + 32 * b + j;                                                   \
            int64_t rowid = -1;                                                                                  \
            if (r < H.n) rowid = H.ids ? (int64_t)H.ids[r] : H.row0 + r;                                         \
            if (rowid < 0) rowid = 0;          /* a skipped entry of the id list: some valid row, result unused */ \
            const T *xp = plane0 + rowid * KP + 8 * h;                                                           \
            _Pragma("unroll") for (int s = 0; s < KS; s++) XB[b][s] = *reinterpret_cast<const V8 *>(xp + 16 * s); \
        }                                                                                                        \
    } while (0)

    // MFMAs of block N_ (accumulator AN) over the drain of block O_'s values (accumulator AO).  The twenty operations of the
    // drain are spread over the MFMAs 1 .. KS-1: block O_'s last MFMA was issued just before this unit's first one, and a
    // drain right behind that one would wait out the matrix pipe's latency.
    // The MFMA intrinsic has no side effects, so neither volatile asm nor sched_barrier orders it (instruction selection sinks
    // it towards its use, behind the drain): two empty asm statements pin it by DATA dependence -- its A operand passes
    // through the first, its result through the second.
#define SEGK_RS_UNIT(XB, N_, AN, O_, AO, REFILL)                                                                     \
    do {                                                                                                              \
        _Pragma("unroll") for (int s = 0; s < KS; s++) {                                                              \
            asm volatile("" : "+v"(a[s]));                                                                            \
            AN = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s], XB[N_][s], s == 0 ? cs : AN, 0, 0, 0);                  \
            asm volatile("" : "+v"(AN));                                                                              \
            if (REFILL && !(SEGK_K1_ABL & 2)) {   /* this tile is done with a[s] (and, after its first MFMA, with cs) */ \
                load_a(tn, s);                                                                                        \
                if (s == 0) load_cs(tn);                                                                              \
            }                                                                                                         \
            __builtin_amdgcn_sched_barrier(0);                                                                        \
            /* quads q_lo .. q_hi-1 of block O_ behind this MFMA: the four quads over the slots 1 .. KS-1 */          \
            constexpr int SL = KS > 1 ? KS - 1 : 1;                                                                   \
            const int q_lo = KS > 1 ? ((s - 1) * 4 + SL - 1) / SL : 0, q_hi = KS > 1 ? (s * 4 + SL - 1) / SL : 4;     \
            if ((KS == 1 || s >= 1) && !(SEGK_K1_ABL & 1)) {                                                          \
                if (0 >= q_lo && 0 < q_hi) SEGK_RS_DRAIN_QUAD(O_, AO, 0, true);                                       \
                if (1 >= q_lo && 1 < q_hi) SEGK_RS_DRAIN_QUAD(O_, AO, 1, false);                                      \
                if (2 >= q_lo && 2 < q_hi) SEGK_RS_DRAIN_QUAD(O_, AO, 2, false);                                      \
                if (3 >= q_lo && 3 < q_hi) SEGK_RS_DRAIN_QUAD(O_, AO, 3, false);                                      \
            }                                                                                                         \
            __builtin_amdgcn_sched_barrier(0);                                                                        \
        }                                                                                                             \
    } while (0)

    // one tile: its two units.  (SEGK_RS_GROUP takes two tiles per trip: with one, the accumulator of the last block and the
    // constants of the next tile change registers across the back edge -- 24 moves and an s_nop 11 per tile)
#define SEGK_RS_TILE(XB, t_)                                        \
    do {                                                            \
        const int tn = (t_) + 1 < nt ? (t_) + 1 : 0;     /* the last tile refills tile 0's operands: the next group's */ \
        SEGK_RS_UNIT(XB, 0, acc0, 1, acc1, false);                  \
        SEGK_RS_UNIT(XB, 1, acc1, 0, acc0, true);                   \
    } while (0)

    // one group: all the range's tiles against the rows in XB, then the (m1, m2) of its rows
#define SEGK_RS_GROUP(g_, XB)                                                                                             \
    do {                                                                                                                   \
        float m1[NBLK], m2[NBLK];                                                                                          \
        _Pragma("unroll") for (int b = 0; b < NBLK; b++) { m1[b] = NEG_INF_F; m2[b] = NEG_INF_F; }                         \
        f32x16 acc0, acc1;                                                                                                 \
        _Pragma("unroll") for (int q = 0; q < 16; q++) acc1[q] = NEG_INF_F;        /* "last block of tile -1": drains to nothing */ \
        int t = 0;                                                                                                         \
        for (; t + 1 < nt; t += 2) {                                                                                       \
            SEGK_RS_TILE(XB, t);                                                                                           \
            SEGK_RS_TILE(XB, t + 1);                                                                                       \
        }                                                                                                                  \
        if (t < nt) SEGK_RS_TILE(XB, t);                                                                                   \
        SEGK_RS_DRAIN_QUAD(NBLK - 1, acc1, 0, true);                                                                       \
        SEGK_RS_DRAIN_QUAD(NBLK - 1, acc1, 1, false);                                                                      \
        SEGK_RS_DRAIN_QUAD(NBLK - 1, acc1, 2, false);                                                                      \
        SEGK_RS_DRAIN_QUAD(NBLK - 1, acc1, 3, false);                                                                      \
        /* the two lane halves of a row hold 16 components of every tile each: merge; stored at the start of the next */   \
        /* group (SEGK_RS_STORE), behind that group's prefetch: a store issued here would sit in front of the loads in */  \
        /* the in-order vmcnt queue and every wait for rows would wait out its write acknowledge as well              */  \
        _Pragma("unroll") for (int b = 0; b < NBLK; b++) {                                                                 \
            const float o1 = __shfl_xor(m1[b], 32), o2 = __shfl_xor(m2[b], 32);                                            \
            pend1[b] = fmaxf(m1[b], o1);                                                                                   \
            pend2[b] = fmaxf(fminf(m1[b], o1), fmaxf(m2[b], o2));                                                          \
        }                                                                                                                  \
        pend_g = (g_);                                                                                                     \
    } while (0)

    // results of the group before: (m1, m2) of its rows (lane half 0)
#define SEGK_RS_STORE()                                                                                                    \
    do {                                                                                                                   \
        if (pend_g >= 0) {                                                                                                 \
            _Pragma("unroll") for (int b = 0; b < NBLK; b++) {                                                             \
                const int64_t r = pend_g * (32 * NBLK) + 32 * b + j;                                                       \
                if (h == 0 && r < H.n && !(H.dbg & 1)) part[(int64_t)range * H.n + r] = make_float2(pend1[b], pend2[b]); \
            }                                                                                                              \
        }                                                                                                                  \
    } while (0)

    V8 a[KS];
    f32x16 cs;
    auto load_a = [&](int t, int s) { a[s] = *reinterpret_cast<const V8 *>((const T *)(lds + t * TL) + (s * 64 + lane) * 8); };
    auto load_cs = [&](int t) {
        const float *cv = lds + t * TL + KS * 256 + 4 * h;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float4 c4 = *reinterpret_cast<const float4 *>(cv + 8 * q);
            cs[4 * q + 0] = c4.x; cs[4 * q + 1] = c4.y; cs[4 * q + 2] = c4.z; cs[4 * q + 3] = c4.w;
        }
    };
    int64_t g = g_first;
    float pend1[NBLK], pend2[NBLK];
    int64_t pend_g = -1;
    V8 xa[NBLK][KS];
    typedef __attribute__((address_space(3))) void *lptr_t;
    if (!is_hint && mm_on && g < n_groups && !(H.dbg & 4)) SEGK_RS_LOAD(g, xa);      // the first rows are requested in front of the tile images (the wait for those, below, covers them)
#ifdef SEGK_STAMP
    const unsigned long long st_k1 = __builtin_amdgcn_s_memtime();
#endif
    // ---- the range's tile images into LDS, once.  The unit of the copy is one 1 KiB piece-0 block (a k-step of a tile:
    // 64 lanes x 16 bytes, contiguous in both images): wave w takes the blocks w, w + SEGK_K1_NW, ...; source and destination of a
    // block are wave-uniform (scalar arithmetic), and ALL of a wave's loads -- 28 for the headline model -- are in flight
    // together: one round trip for the 114 KB.  (Element-wise with a division per 16 bytes and 16 loads in flight per thread
    // the fill took 21 700 cycles, 12 us of a 200 us kernel -- and a third of a 1 250-utterance shard's.)
    {
        constexpr int MAXT = (160 * 1024 / (TL * 4)) < SEGK_HINT_MAX_TPR ? (160 * 1024 / (TL * 4)) : SEGK_HINT_MAX_TPR;
        constexpr int MAXB = MAXT * KS;                                 // blocks of the largest range (LDS, SEGK_HINT_MAX_TPR)
        constexpr int NWF = 2 * SEGK_K1_NW;                                     // all eight waves copy
        constexpr int PER_W = (MAXB + NWF - 1) / NWF;
        const int n_blk = nt * KS;
        // every workgroup of a range copies the same bytes at the same moment: started at the same block they all queue on
        // the same L2 channel (5.8 bytes per cycle and CU measured).  Each starts somewhere else in the range instead.
        const int rot = (int)(((unsigned)wgr * 2654435761u) >> 8) % n_blk;
        // (a block lands in LDS as it lies in the image, 16 bytes per lane: LDS-DMA, no register in between; the wave waits
        // for its own pieces in front of the barrier)
        const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lptr_t)lds);
#pragma unroll
        for (int u = 0; u < PER_W; u++) {
            int c = wave + u * NWF;
            if (mm_on && c < n_blk) {
                c += rot;
                if (c >= n_blk) c -= n_blk;
                const int t = __builtin_amdgcn_readfirstlane(c / KS), ks = __builtin_amdgcn_readfirstlane(c) - t * KS;
                const float *src = tiles + (int64_t)(t_lo + t) * STRIDE + ks * (P * 256) + lane * 4;
                const unsigned dst = lds0 + (unsigned)(t * TL + ks * 256) * 4u;
                unsigned keep_;
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                             "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep_)
                             : "v"(src), "s"(dst)
                             : "memory");
            }
        }
        float4 cv4 = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool has_c = mm_on && tid < nt * 8;                       // the 32 constants of every tile: one float4 per thread
        if (has_c) cv4 = *reinterpret_cast<const float4 *>(tiles + (int64_t)(t_lo + (tid >> 3)) * STRIDE + KS * P * 256 + (tid & 7) * 4);
        // the label map of the hint waves behind the tile images
        int32_t *map_l = reinterpret_cast<int32_t *>(lds + map_off);
        // the label a hint of the previous call stands for now (the relabelling of clean_components), or -1 when the
        // filters' images carry that component as absent (seed constant <= -1e37, a marked duplicate: such a hint proves nothing)
        for (int k = tid; k < H.K_max; k += 128 * SEGK_K1_NW) {
            int v = H.remap ? H.remap[k] : k;
            if (v < 0 || v >= H.K_max) v = -1;
            else if (H.full.tiles[(int64_t)(v >> 5) * STRIDE + KS * P * 256 + (v & 31)] < -1.0e37f) v = -1;
            if (skip_ok && v >= 0 && H.meanchg[v]) v |= SEGK_MEANCHG_BIT;
            map_l[k] = v;
        }
        if (has_c) *reinterpret_cast<float4 *>(lds + (tid >> 3) * TL + KS * 256 + (tid & 7) * 4) = cv4;
        static_assert(128 * SEGK_K1_NW >= MAXT * 8, "one thread per float4 of the constants");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (is_hint) {
        // a full launch of the delta score pass is the new base: the first workgroup of every range leaves the image it
        // multiplies (its LDS, the snapshot's layout) for k_delta_prep to compare the next calls' images with
        if (H.ctl && !delta && mm_on && wgr == 0) {
            float4 *dst = reinterpret_cast<float4 *>(H.snap_img + 4 + (int64_t)t_lo * TL);
            const float4 *src = reinterpret_cast<const float4 *>(lds);
            for (int i = tid - 64 * SEGK_K1_NW; i < nt * (TL / 4); i += 64 * SEGK_K1_NW) dst[i] = src[i];
        }
        // every workgroup's hint waves take steps of 32 rows, strided over the whole grid: the chip walks the corpus front to back
        hint_wave_rows<KS, V>(H, reinterpret_cast<const int32_t *>(lds + map_off), (int64_t)blockIdx.x * SEGK_K1_NW + (wave - SEGK_K1_NW),
                              (int64_t)grid * SEGK_K1_NW, skip_ok);
        return;
    }
#ifdef SEGK_STAMP
    const unsigned long long st_k2 = __builtin_amdgcn_s_memtime();
#endif
    if (!mm_on || g >= n_groups || (H.dbg & 128)) return;       // (dbg 128, make DEV=1: timing of the hint waves alone)
    if (H.dbg & 4) SEGK_RS_LOAD(g, xa);
#pragma unroll
    for (int s = 0; s < KS; s++) load_a(0, s);          // tile 0's operands for the first group; every group's last tile reloads them
    load_cs(0);
    V8 xb[NBLK][KS];                                    // the second register set: groups alternate between xa and xb
    // The explicit waits (the builtin, which the compiler's wait-count pass understands; an asm wait it would not) tell
    // it that the current set has landed BEFORE the other set's loads are issued: left to itself it waits for the
    // current set inside the tile loop with counted vmcnt, which -- the counter being in issue order -- waits out the
    // prefetch too.  What is outstanding at such a wait was issued a whole group earlier (the rows, the stores of the
    // group before).
#ifdef SEGK_STAMP
    unsigned long long st_wait = 0, st_loop = 0, st_groups = 0;
    const unsigned long long st_begin = __builtin_amdgcn_s_memtime();
#define SEGK_ST(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#else
#define SEGK_ST(var) do { } while (0)
#endif
    for (;;) {
        SEGK_ST(s0);
        __builtin_amdgcn_s_waitcnt(0x0F70);                             // vmcnt(0): the rows of group g are in xa
        SEGK_ST(s1);
        const int64_t g1 = g + n_slots;
        if (g1 < n_groups) SEGK_RS_LOAD(g1, xb);          // in flight under this group's tile loop
        SEGK_RS_STORE();
        SEGK_ST(s2);
        SEGK_RS_GROUP(g, xa);
        SEGK_ST(s3);
#ifdef SEGK_STAMP
        st_wait += s1 - s0; st_loop += s3 - s2; st_groups++;
#endif
        if (g1 >= n_groups) break;
        SEGK_ST(s4);
        __builtin_amdgcn_s_waitcnt(0x0F70);
        SEGK_ST(s5);
        g = g1 + n_slots;
        if (g < n_groups) SEGK_RS_LOAD(g, xa);
        SEGK_RS_STORE();
        SEGK_ST(s6);
        SEGK_RS_GROUP(g1, xb);
        SEGK_ST(s7);
#ifdef SEGK_STAMP
        st_wait += s5 - s4; st_loop += s7 - s6; st_groups++;
#endif
        if (g >= n_groups) break;
    }
#ifdef SEGK_STAMP
    if (H.stamp && lane == 0) {
        unsigned long long *o = H.stamp + ((int64_t)blockIdx.x * SEGK_K1_NW + wave) * 8;
        o[0] = st_wait; o[1] = st_loop; o[2] = __builtin_amdgcn_s_memtime() - st_begin; o[3] = st_groups;
        o[4] = st_begin - st_k0; o[5] = st_r0; o[6] = __builtin_amdgcn_s_memrealtime(); o[7] = ((st_k1 - st_k0) << 32) | (st_k2 - st_k1);
    }
#endif
#undef SEGK_ST
    SEGK_RS_STORE();
    if (fb && lane == 0) atomicMax(&H.fb_t[H.fb_cur * 8 + (blockIdx.x & 7)], (unsigned int)(__builtin_amdgcn_s_memrealtime() - fb_t0));
#undef SEGK_RS_STORE
#undef SEGK_RS_GROUP
#undef SEGK_RS_TILE
#undef SEGK_RS_UNIT
#undef SEGK_RS_LOAD
}
#undef SEGK_RS_DRAIN_QUAD

// ---- delta score pass: what changed since the base pass ------------------------------------------------------------------
// One small launch in front of K1.  A workgroup per tile: every column of the image K1 multiplies (piece 0 of every k-step and the
// constant, "absent" marks included) against the snapshot of the base pass, bit for bit; a changed image exponent changes the
// scale of every filter value and so marks every column.  The changed columns are compacted into the leading tiles of the packed
// delta image (any order: K1 keeps values, not indices; the free slots of the last tile carry the absent constant), and the mode
// word says which parameter set K1's launch takes: FULL when there is no valid state, when the relabelling is not the identity, or when
// the packed tiles exceed `cap` -- and then K1 in full mode, which makes the new base, refreshes the snapshot.
// A base is never built from delta results, so the changed columns only accumulate against the snapshot; two more reasons for a
// full launch bring them back down: the chain has come to rest on changed columns (no new column in this call and no mean moved
// during the previous one: one full pass, and every later call multiplies nothing), or the packed tiles multiplied since the base
// add up to a whole table (the delta passes have then cost what the new base costs).
// The workgroups behind the tiles': the rows of the float32 `means` against their copy of the previous call (a wave per row),
// for the hint waves, and the copy refreshed.
// (DeltaPrepArgs and the three bodies -- delta_prep_tile, delta_prep_means_rows, delta_prep_mode -- are in segk_kmeans_dev.h:
// k_batch_post runs them too, for the hinted call that follows a batch finalize.)
// Workgroups 0 .. n_tiles - 1: one tile each; the workgroup that finishes last knows the count and writes the mode.  The
// snapshot itself is refreshed by K1's full launch, which has every tile in LDS anyway.  The workgroups behind: the rows of
// `means`.  This launch is the path of every hinted call that has no pending prep (launch_delta_prep).
template <int KS>
__global__ __launch_bounds__(SEGK_PREP_THREADS) void k_delta_prep(DeltaPrepArgs P)
{
    if ((int)blockIdx.x >= P.n_tiles) {
        delta_prep_means_rows(P, (int)blockIdx.x - P.n_tiles, (int)gridDim.x - P.n_tiles);
        return;
    }
    __shared__ DeltaPrepLds S;
    const int e_cur = ((const int *)P.tiles_hdr)[0];
    if (delta_prep_tile(P, KS, (int)blockIdx.x, e_cur, S)) delta_prep_mode(P, KS, e_cur, S);
}

struct HintMergeArgs {
    const float2 *part;             // K1's matrix waves: (m1, m2) per (range, position)
    const float4 *hint_out;         // K1's hint waves: {s, f_h, bits of h, 0} per position
    int n_ranges;
    const float *tiles_hdr;         // tiles_b3: [0] exponent b, [1] E_m
    const unsigned char *ximg;      // row image header: [1] exponent a
    // delta score pass (ctl NULL: none)
    const int32_t *ctl;
    const float2 *part_delta;       // (m1, m2) per position over the packed changed columns
    int32_t *lab_base;              // per position: the label the base pass certified, or -1
    const int32_t *colchg;          // per column: its image differs from the base pass's
    const int32_t *meanchg;         // per row of `means`: its bits changed since the previous call
    int32_t *lab_last;              // per position: the label this library decided in the previous call, or -1 (the carry-over)
    int32_t *stats_host;            // host-mapped [4] (segk_kmeans_delta_stats)
};

// K2 (round 4): the certificate.  Per row the filter's top-2 merged over the ranges, the hinted component's exact score s and its
// filter-domain value f_h (see the head of the file):
//     top1 - top2 > tau   and   f_h >= top1 - tau + E + dl      =>   cand.k = h, cand.s = s  (the reference's bits)
// anything else -- no hint, a wrong hint, a near-tie -- is queued for the second stage (one reservation per wave), unless the
// call is a delta call and the row's winner of the previous call carries over the unchanged means (head of the file: no base
// value enters that test, only the changed columns' maximum and f_h).  One thread
// per row, 48 bytes read and 12 written (with delta state 4 more each way for lab_last, the store only where it changes): the whole exact stage of round 3 (k_kmeans_hint_exact, 129 us) shrunk to this pass,
// its arithmetic moved under K1's matrix work.
#define SEGK_MERGE_ROWS 6144        /* rows per workgroup at most (its list of undecided rows in LDS) */
#define SEGK_MERGE_THREADS 1024
__global__ __launch_bounds__(SEGK_MERGE_THREADS) void k_hint_merge(ScoreArgs A, HintMergeArgs H, int KP, int64_t per, float *pre_thr, int64_t first_skipped)
{
    // ONE queue reservation per workgroup, one workgroup per CU: returning atomics on one address are served one after the other,
    // ~11 ns each (a first version with one per wave -- 15 600 of them -- took 185 us for 55 MB of traffic, 1 024 workgroups
    // still 25 us); the workgroup's undecided rows wait in LDS
    __shared__ int32_t ulist[SEGK_MERGE_ROWS];
    __shared__ float uthr[SEGK_MERGE_ROWS];         // per undecided row: top1 - tau in the scaled domain (the band stage's threshold)
    __shared__ int32_t ucnt, ubase;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) ucnt = 0;
    // delta score pass.  In delta mode `part` is still the BASE pass's (m1, m2): values of the columns as they were then.  For a
    // column whose image has not changed that is its current filter value F_k; for a changed one it is stale, and the current
    // value is in part_delta.  The certificate holds on such a superset (head of the file): the stale values can only make it
    // fail.  One case is worth repairing: the row's hint h is the label the base pass certified (lab_base) and column h has
    // changed.  Then the base's largest value over all ranges is the stale F_h -- the certificate made it the single largest --,
    // and with it in the set the fresh F_h could never lead by tau.  Drop it: every OTHER column's base value is at most the
    // base's second largest t2 (the larger of the ranges' m2 and of their m1 but the largest), so {t2, t2} stands for all of them
    // (a value >= F_k for every unchanged k != h; the changed ones have their current value in part_delta, F_h among them).
    const int mw = H.ctl ? H.ctl[0] : 0;
    const bool delta = (mw & SEGK_DELTA_MODE) != 0;
    const int n_chg = H.ctl ? H.ctl[1] : 0, n_packed = H.ctl ? H.ctl[2] : 0;
    if (H.stats_host && blockIdx.x == 0 && tid == 0) {
        H.stats_host[1] = n_chg;
        H.stats_host[2] = n_packed;
        H.stats_host[3] = H.ctl ? H.ctl[3] : 0;
        __hip_atomic_store(H.stats_host, H.ctl ? 1 + (delta ? 1 : 0) : 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __syncthreads();
    // the carry-over (head of the file), conditions 1 and 4: per call, the same answer in every workgroup -- the two flag arrays
    // are 8 KB from L2.  A changed mean whose column is not packed switches it off unless the current image marks it absent.
    bool carry = false;
    if (delta && (mw & SEGK_DELTA_SKIP) != 0 && H.lab_last) {              // (workgroup-uniform)
        const int c_off = (KP / 16) * 512;
        bool bad = false;
        for (int k = tid; k < A.K_max; k += SEGK_MERGE_THREADS)
            if (H.meanchg[k] && !H.colchg[k])
                bad |= !(H.tiles_hdr[1024 + (int64_t)(k >> 5) * A.tile_stride + c_off + (k & 31)] < -1.0e37f);
        carry = __syncthreads_or(bad ? 1 : 0) == 0;
    }
    const int64_t p_lo = (int64_t)blockIdx.x * per, p_hi = p_lo + per < A.n ? p_lo + per : A.n;
    const int e_ab = ((const int *)H.ximg)[1] + ((const int *)H.tiles_hdr)[0];
    const float unscale = ldexpf(1.f, -e_ab), scale = ldexpf(1.f, e_ab);
    const float M = (float)(sqrt(*A.mnorm2) * (1.0 + 1e-6)) + 1e-30f;
    const float Em = H.tiles_hdr[1];
    // five rows per thread and trip, their loads in flight together (one row per trip was four dependent round trips per
    // workgroup: 25 us for 55 MB; with four the headline corpus -- 4 102 rows per workgroup -- took a second trip for six rows)
    constexpr int U = 5;
    for (int64_t p0 = p_lo; p0 < p_hi; p0 += SEGK_MERGE_THREADS * U) {
        int32_t rid[U];
        float4 ho[U];
        float t1[U], t2[U], xnb[U], xer[U], d1[U];
        int32_t last[U];                // lab_last of the position where the carry-over is on (else -2: matches no hint, no label)
        bool cw[U];                     // conditions 2 and 3 of the carry-over hold for the row
#pragma unroll
        for (int j = 0; j < U; j++) {
            const int64_t p = p0 + j * SEGK_MERGE_THREADS + tid;
            rid[j] = -1;
            if (p < p_hi) rid[j] = A.ids ? A.ids[p] : (int32_t)(A.row0 + p);
        }
#pragma unroll
        for (int j = 0; j < U; j++) {
            const int64_t p = p0 + j * SEGK_MERGE_THREADS + tid;
            ho[j] = make_float4(0.f, 0.f, __int_as_float(-1), 0.f);
            t1[j] = NEG_INF_F; t2[j] = NEG_INF_F; xnb[j] = 0.f; xer[j] = 0.f;
            if (rid[j] >= 0) {
                ho[j] = H.hint_out[p];
                for (int r = 0; r < H.n_ranges; r++) {
                    const float2 pv = H.part[(int64_t)r * A.n + p];
                    const float n1 = fmaxf(t1[j], pv.x);
                    t2[j] = fmaxf(fminf(t1[j], pv.x), fmaxf(t2[j], pv.y));
                    t1[j] = n1;
                }
                xnb[j] = A.xnorm[rid[j]];
                xer[j] = A.xerr[rid[j]];
            }
            d1[j] = NEG_INF_F;
            last[j] = -2;
            cw[j] = false;
            if (rid[j] >= 0 && carry) {
                const int32_t hint = __float_as_int(ho[j].z);
                last[j] = H.lab_last[p];
                cw[j] = hint >= 0 && last[j] == hint && H.meanchg[hint] == 0;
            }
            if (rid[j] >= 0 && delta) {
                const int32_t hint = __float_as_int(ho[j].z);
                if (hint >= 0 && H.colchg[hint] && H.lab_base[p] == hint) {
                    t1[j] = t2[j];
                }
                if (n_packed > 0) {
                    const float2 pv = H.part_delta[p];
                    d1[j] = pv.x;
                    const float n1 = fmaxf(t1[j], pv.x);
                    t2[j] = fmaxf(fminf(t1[j], pv.x), fmaxf(t2[j], pv.y));
                    t1[j] = n1;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < U; j++) {
            bool und = false;
            float thr = 0.f;
            int32_t keep = -1;          // what lab_last gets: the label decided here, -1 for a row that goes on
            if (rid[j] >= 0 && p0 + j * SEGK_MERGE_THREADS + tid >= first_skipped) {
                // a row K1 left out (the few groups behind the last whole round of its waves): no filter values, full scan
                const int q2 = atomicAdd(A.cand.count, 1);
                if (q2 < A.amb_cap) A.cand.queue[q2] = rid[j];
            } else if (rid[j] >= 0) {
                const int32_t hint = __float_as_int(ho[j].z);
                und = true;
                const float tau = filter_tau_h1(xnb[j], M, A.D, xer[j], Em);
                // the band the reference's argmax lies in: F >= top1 - tau (scaled domain; the subtraction's own rounding and a
                // little more taken off)
                // (delta mode with changed columns: t1 may be a stale value, no bound on anything -- below)
                float lower = t1[j];
                thr = t1[j] - tau * scale * 1.000001f;
                thr -= 4e-7f * fabsf(t1[j]);
                bool ok = false;
                if (hint >= 0) {
                    const float top1 = t1[j] * unscale, top2 = t2[j] * unscale;          // powers of two: exact
                    const float u = 5.9604645e-8f;
                    // E: bound of |F_k - f_k| (accumulation + operand rounding, the terms of tau); dl: of the computed f_h
                    const float e1 = (1.02f * (float)(KP + 16) + 16.f) * u * (xnb[j] * M + 0.5f * M * M);
                    const float rnd = 1.00001f * fminf((xnb[j] + xer[j]) * Em + xer[j] * M, 1.01f * 9.765625e-4f * xnb[j] * M);
                    const float s2 = xnb[j] + M;
                    const float dl = ((float)(A.D / 8 + 13) + 4.f) * u * s2 * s2;
                    ok = (top1 - top2 > tau) && (ho[j].y >= top1 - tau + (e1 + rnd + dl) * 1.0001f);
                    // the carry-over, condition 5: every changed mean's current filter value (at most d1) leaves f_h the slack the
                    // certificate leaves a competitor; d1 = -inf where nothing is packed
                    const bool carried = !ok && cw[j] && ho[j].y > d1[j] * unscale + (e1 + rnd + dl) * 1.0001f;
                    if (ok || carried) {
                        A.cand.k[rid[j]] = hint;
                        A.cand.s[rid[j]] = (double)ho[j].x;
                        und = false;
                        keep = hint;
                    }
                    // the current F_h is at least f_h - E - dl: a lower bound of the current top1 whatever the base holds
                    lower = (ho[j].y - (e1 + rnd + dl) * 1.0001f) * scale;
                    lower -= 4e-7f * fabsf(lower);
                }
                if (H.lab_base && !delta) H.lab_base[p0 + j * SEGK_MERGE_THREADS + tid] = ok ? hint : -1;
                if (und && delta && n_chg > 0) {
                    // The band threshold must stay a LOWER bound of (current top1) - tau.  Current values this row has: those of
                    // the changed columns (d1, their largest) and the bound from the hinted score; a lower threshold only yields
                    // more candidates.  Without a hint there is no usable bound: the full scan.
                    if (hint < 0) {
                        und = false;
                        const int q2 = atomicAdd(A.cand.count, 1);
                        if (q2 < A.amb_cap) A.cand.queue[q2] = rid[j];
                    } else {
                        lower = fmaxf(lower, d1[j]);
                        thr = lower - tau * scale * 1.000001f;
                        thr -= 4e-7f * fabsf(lower);
                    }
                }
            }
            // every position, every call with delta state (full mode too); k_band_exact puts its winner over the -1 of a queued row
            if (H.lab_last && rid[j] >= 0 && last[j] != keep) H.lab_last[p0 + j * SEGK_MERGE_THREADS + tid] = keep;
            const unsigned long long mask = __ballot(und);
            if (mask != 0ull) {
                const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
                int base = 0;
                if (lane == 0) base = atomicAdd(&ucnt, __popcll(mask));           // LDS
                base = __shfl(base, 0);
                if (und) {
                    ulist[base + before] = rid[j];
                    uthr[base + before] = thr;
                }
            }
        }
    }
    __syncthreads();
    const int cnt = ucnt;
    if (cnt == 0) return;
    if (tid == 0) ubase = atomicAdd(A.pre_count, cnt);
    __syncthreads();
    const int base = ubase;
    for (int i = tid; i < cnt; i += SEGK_MERGE_THREADS) {
        const int q = base + i;
        const int32_t rid = ulist[i];
        if (q < A.pre_cap) {
            A.pre_queue[q] = rid;
            if (pre_thr) pre_thr[q] = uthr[i];
        } else {                                               // beyond the second stage's launch: full scan
            const int q2 = atomicAdd(A.cand.count, 1);
            if (q2 < A.amb_cap) A.cand.queue[q2] = rid;
        }
    }
}

// ---- host side: workspaces -> plan -> delta prep -> K1 -> merge -> second stage ---------------------------------------------
// How one call is laid out over K1
struct HintLaunch {
    HintPlan lds;                   // the LDS ranges of a full launch
    bool band;                      // the band stage takes the undecided rows (else: the three-product second stage)
    int grid;                       // a full launch's workgroups
    int64_t k1_groups;              // row groups K1 multiplies; the rows from k1_groups * 64 on take the full scan
    float *fb_w;                    // the XCD shares' three slots, this call's slot (k1_xcd_share)
    unsigned int *fb_t;             // NULL: equal shares
    int fb_cur;
    float4 *hint_out;               // the hint waves' result, behind the matrix waves' in hint_part
    bool part_fresh;                // hint_part has just been reallocated: it holds no base pass
};

// The second stage's queue (as the pre-filter path) and its thresholds, K1's partial top-2 and hint scores, the XCD shares
static int hint_workspaces(segk_ctx *ctx, ScoreArgs &A, HintLaunch &L, hipStream_t st)
{
    if (int rc = segk_ws_grow(ctx, &ctx->pre_queue, &ctx->pre_cap, A.n, sizeof(int32_t) * (size_t)(A.n + 16), st)) return rc;
    A.pre_queue = ctx->pre_queue + 16;
    A.pre_count = ctx->pre_queue;
    A.pre_cap = (int)A.n;
    if (L.band)
        if (int rc = segk_ws_grow(ctx, &ctx->pre_thr, &ctx->pre_thr_cap, A.n, sizeof(float) * (size_t)A.n, st)) return rc;
    // [n_ranges][n] (m1, m2) of the matrix waves, then [n] {s, f_h, h, 0} of the hint waves
    const size_t part_bytes = ((size_t)L.lds.n_ranges * (size_t)A.n * sizeof(float2) + 255) & ~(size_t)255;
    const size_t need_part = part_bytes + (size_t)A.n * sizeof(float4);
    L.part_fresh = ctx->hint_part_bytes < need_part;
    if (int rc = segk_ws_grow(ctx, &ctx->hint_part, &ctx->hint_part_bytes, need_part, need_part, st)) return rc;
    L.hint_out = (float4 *)((unsigned char *)ctx->hint_part + part_bytes);
    // per-XCD shares of the row groups (k1_xcd_share): three slots of (shares, lifetimes), owned by the context
    if (!ctx->hint_fb) {
        float init[3 * 8 + 3 * 8];
        SEGK_CHECK_HIP(hipMalloc(&ctx->hint_fb, sizeof(init)));
        for (int i = 0; i < 24; i++) init[i] = 0.125f;
        memset(init + 24, 0, 24 * sizeof(unsigned int));
        SEGK_CHECK_HIP(hipMemcpyAsync(ctx->hint_fb, init, sizeof(init), hipMemcpyHostToDevice, st));
        SEGK_CHECK_HIP(hipStreamSynchronize(st));                            // (`init` lives on this stack frame)
        ctx->hint_fb_launch = 0;
    }
    return SEGK_OK;
}

// A full launch's grid, the XCD shares' slot, and the row groups K1 multiplies
static void hint_plan_rows(segk_ctx *ctx, const ScoreArgs &A, HintLaunch &L)
{
    const int n_ranges = L.lds.n_ranges;
    const int64_t total_groups = (A.n + 63) / 64;                // K1: two blocks of 32 rows per group
    L.fb_w = (float *)ctx->hint_fb;
    // (only where a wave has a few dozen groups to shift: at shard sizes -- 4 to 8 groups of 5 us per wave -- shares other
    // than equal ones only make the last round ragged: 1 250 utterances 5 960 against 6 215 sweeps/s, 2 500: 4 878 against 4 948)
    const bool fb_big = total_groups >= 192 * 64;
    L.fb_t = (segk_env_int("SEGK_HINT_BALANCE", 1) == 0 || !fb_big) ? nullptr : (unsigned int *)(L.fb_w + 24);
    L.fb_cur = (int)(ctx->hint_fb_launch++ % 3u);
    // one workgroup per CU in whole sets of ranges, no more than there are steps per range (a workgroup's four matrix waves
    // take 64 rows each at a time)
    L.grid = (ctx->n_cu / n_ranges) * n_ranges;
    const int64_t steps = (A.n + 64 * SEGK_K1_NW - 1) / (64 * SEGK_K1_NW);
    if ((int64_t)L.grid / n_ranges > steps) L.grid = (int)steps * n_ranges;
    // With equal shares every wave walks the groups slot, slot + slots, ...: when a handful of groups is left behind the last
    // whole round (a 1 250-utterance shard: 2 051 groups = 4 x 512 + 3) three waves would take a fifth group, 5 us, for all
    // the others to wait on.  Those few rows skip the filter: k_hint_merge sends them to the full scan.
    // (in front of the band stage that is 9 us for a shard's 192 rows: no skipping then)
    L.k1_groups = total_groups;
    if (!L.fb_t && !L.band) {
        const int64_t slots = (int64_t)(L.grid / n_ranges) * SEGK_K1_NW;
        const int64_t whole = slots > 0 ? (total_groups / slots) * slots : 0;
        if (whole > 0 && total_groups - whole <= 32) L.k1_groups = whole;
    }
}

// ---- delta score pass: K1's (m1, m2) of the last FULL launch stay in hint_part as the base; while the call tuple repeats,
// k_delta_prep finds the columns whose image changed since and K1 multiplies those alone.
// Its state, one allocation (ctx->delta_buf); every part starts on a 256-byte boundary:
struct DeltaBuf {
    int32_t *ctl;                   // [64] control words (see SEGK_DELTA_MODE); NULL: no delta pass in this call
    int32_t *colchg, *meanchg;      // per column of the image / row of `means`: changed
    float *snap_img;                // the base pass's image [4 floats: exponent][n_tiles][KS * 256 + 32]
    float *packed;                  // the packed image of the changed columns [n_tiles][stride]
    float *snap_means;              // the previous call's `means` [K_max][D]
    float2 *part;                   // [n] (m1, m2) over the packed columns
    int32_t *lab_base;              // [n] the label the base pass certified, or -1
    int32_t *lab_last;              // [n] the label the previous call decided for the position (a certificate, the carry-over, or the
                                    // band stage), or -1: the full scan did, or the row was not covered
    size_t zero_bytes;              // what a fresh allocation must have cleared: everything in front of snap_means
};
// the parts of a buffer at `b` (NULL: the sizes only); returns its bytes
static size_t delta_layout(unsigned char *b, int n_tiles, int K_max, int D, int64_t n, int stride, DeltaBuf *B)
{
    const size_t TL = (size_t)(segk_b3_kp(D) / 16) * 256 + 32;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        unsigned char *p = b ? b + off : nullptr;
        off += (bytes + 255) & ~(size_t)255;
        return p;
    };
    B->ctl = (int32_t *)take(256);
    B->colchg = (int32_t *)take((size_t)n_tiles * 32 * 4);
    B->meanchg = (int32_t *)take((size_t)K_max * 4);
    B->snap_img = (float *)take(((size_t)n_tiles * TL + 4) * 4);
    B->packed = (float *)take((size_t)n_tiles * stride * 4);
    B->zero_bytes = off;
    B->snap_means = (float *)take((size_t)K_max * D * 4);
    B->part = (float2 *)take((size_t)n * 8);
    B->lab_base = (int32_t *)take((size_t)n * 4);
    B->lab_last = (int32_t *)take((size_t)n * 4);
    return off;
}

// packed tiles a delta launch takes at most: a full launch's range (measured on the headline corpus against 2, 4, 8, 12 and 20
// tiles: profiles/README.md), never more than fit in K1's LDS; and the packed tiles multiplied since the base at most
static int delta_cap(const HintPlan &lds)
{
    int cap = segk_env_int("SEGK_DELTA_CAP", lds.tpr);
    if (cap > lds.max_tiles) cap = lds.max_tiles;
    return cap < 1 ? 1 : cap;
}
static int delta_budget(int n_tiles) { return segk_env_int("SEGK_DELTA_BUDGET", n_tiles); }

// the prep's arguments for a table on the buffer B; consumes a launch number of the context unless it repeats launch redo_seq
static DeltaPrepArgs delta_prep_args(segk_ctx *ctx, const DeltaBuf &B, const float *tiles, int n_tiles, int stride, int K_max, int D,
                                     const float *means32, const int32_t *remap, const int32_t *K_dev, bool valid, int cap, int budget,
                                     int redo_seq = -1)
{
    DeltaPrepArgs P{};
    P.tiles_hdr = tiles; P.n_tiles = n_tiles; P.stride = stride;
    P.K_max = K_max; P.D = D; P.means32 = means32; P.remap = remap; P.K_dev = K_dev;
    P.valid = valid ? 1 : 0; P.hint_valid = valid ? 1 : 0; P.cap = cap;
    P.budget = budget;
    P.redo = redo_seq >= 0 ? 1 : 0;
    P.seq = redo_seq >= 0 ? redo_seq : (int)(ctx->delta_seq++ & 1u);
    P.ctl = B.ctl; P.colchg = B.colchg; P.meanchg = B.meanchg;
    P.snap_img = B.snap_img; P.packed = B.packed; P.snap_means = B.snap_means;
    return P;
}

// segk_kmeans_batch_finalize: k_batch_post has just finished the images and follows the kernel that wrote `means` -- it runs
// the prep of the next hinted call on this table if the context holds valid delta state for it: the previous hinted call was
// on this table over all rows (its key), the buffer is that call's, nothing is pending.  The arguments are those the call's
// own launch_delta_prep would make (state valid); it takes the prep over if it finds them so, and has no valid state if not.
// SEGK_DELTA_PREP_FOLD=0: never (same results).
bool segk_delta_prep_fold(segk_ctx *ctx, const segk_corpus *c, const segk_kmeans *m, const int32_t *remap, hipStream_t st, DeltaPrepArgs *P)
{
    *P = DeltaPrepArgs{};
    if (!ctx || ctx->delta_pending != 0 || !ctx->delta_valid || ctx->capturing || !ctx->delta_buf) return false;
    if (segk_env_int("SEGK_DELTA_PREP_FOLD", 1) == 0 || segk_env_int("SEGK_SCORE_DELTA", 1) == 0) return false;
    const void *key[4] = {c->Xb3, c->X32, m->tiles_b3, m->means};
    const int64_t key_n[5] = {0, c->n_emb, c->n_emb, m->K_max, c->D};
    if (memcmp(key, ctx->delta_key, sizeof(key)) != 0 || memcmp(key_n, ctx->delta_key_n, sizeof(key_n)) != 0) return false;
    const int n_tiles = segk_n_tiles(m->K_max), stride_sp = segk_sp_tile_stride(c->D, 2);
    HintPlan lds;
    if (n_tiles > 32 * SEGK_PREP_COLS || !segk_hint_plan(m->K_max, segk_b3_kp(c->D) / 16, n_tiles, &lds)) return false;
    DeltaBuf B{};
    if (ctx->delta_bytes != delta_layout(nullptr, n_tiles, m->K_max, c->D, c->n_emb, stride_sp, &B)) return false;
    delta_layout((unsigned char *)ctx->delta_buf, n_tiles, m->K_max, c->D, c->n_emb, stride_sp, &B);
    const int cap = delta_cap(lds), budget = delta_budget(n_tiles);
    *P = delta_prep_args(ctx, B, m->tiles_b3, n_tiles, stride_sp, m->K_max, c->D, (const float *)m->means, remap, m->K, true, cap, budget);
    ctx->delta_pending = 1;
    ctx->delta_pending_remap = remap; ctx->delta_pending_K = m->K; ctx->delta_pending_stream = (const void *)st;
    ctx->delta_pending_cap = cap; ctx->delta_pending_budget = budget; ctx->delta_pending_seq = P->seq;
    return true;
}

// The prep in front of K1 where the delta pass applies (SEGK_SCORE_DELTA=0: never); B->ctl == NULL where it does not.  A launch
// of k_delta_prep, unless k_batch_post has run this very prep (the context's pending prep).  *cap: packed tiles a delta launch
// takes at most.
template <int KS>
static int launch_delta_prep(segk_ctx *ctx, const ScoreArgs &A, const int32_t *remap, const int32_t *K_dev, int64_t n_emb,
                             const HintLaunch &L, hipStream_t st, DeltaBuf *B, int *cap)
{
    *B = DeltaBuf{};
    *cap = 0;
    const int pending = ctx->delta_pending;                  // consumed by the first hinted call after it, used or not
    ctx->delta_pending = 0;
    const bool delta_on = segk_env_int("SEGK_SCORE_DELTA", 1) != 0 && L.band && A.ids == nullptr && A.n_tiles <= 32 * SEGK_PREP_COLS;
    const void *key[6] = {A.X32, A.xrows32, A.tiles, A.means32, A.cand.k, A.cand.s};
    const int64_t key_n[5] = {A.row0, A.n, n_emb, A.K_max, A.D};
    bool state_valid = delta_on && !L.part_fresh && ctx->delta_valid && memcmp(key, ctx->delta_key, sizeof(key)) == 0 &&
                       memcmp(key_n, ctx->delta_key_n, sizeof(key_n)) == 0;
    ctx->delta_valid = 0;
    if (!delta_on) return SEGK_OK;
    const int stride_sp = segk_sp_tile_stride(A.D, 2);
    const size_t need = delta_layout(nullptr, A.n_tiles, A.K_max, A.D, A.n, stride_sp, B);
    if (ctx->delta_bytes != need) {
        ctx->delta_bytes = 0;
        if (int rc = segk_ws_realloc(ctx, &ctx->delta_buf, need, st)) return rc;
        ctx->delta_bytes = need;
        state_valid = false;
        // (the packed image's free slots must hold finite operands: zero now, copies of real columns ever after)
        SEGK_CHECK_HIP(hipMemsetAsync(ctx->delta_buf, 0, B->zero_bytes, st));
    }
    delta_layout((unsigned char *)ctx->delta_buf, A.n_tiles, A.K_max, A.D, A.n, stride_sp, B);
    *cap = delta_cap(L.lds);
    const int budget = delta_budget(A.n_tiles);
    // the pending prep is this call's: made for this tuple (state_valid: the key it was made from), this relabelling table and
    // component count, this stream, these limits.  One that is not -- or was dropped after it ran -- has refreshed the means'
    // snapshot and moved the counters on all the same: on valid state (its own: only the hinted call of the key sets one up,
    // and every hinted call consumes it) the launch repeats it.  Without valid state k_delta_prep resets every control word.
    const bool folded = pending == 1 && state_valid && remap == ctx->delta_pending_remap && K_dev == ctx->delta_pending_K &&
                        (const void *)st == ctx->delta_pending_stream && *cap == ctx->delta_pending_cap &&
                        budget == ctx->delta_pending_budget;
    if (!folded) {
        const DeltaPrepArgs P = delta_prep_args(ctx, *B, A.tiles, A.n_tiles, stride_sp, A.K_max, A.D, A.means32, remap, K_dev, state_valid,
                                                *cap, budget, pending != 0 && state_valid ? ctx->delta_pending_seq : -1);
        hipLaunchKernelGGL(k_delta_prep<KS>, dim3(A.n_tiles + segk_delta_prep_row_blocks(A.K_max)), dim3(SEGK_PREP_THREADS), 0, st, P);
    }
    memcpy(ctx->delta_key, key, sizeof(key));
    memcpy(ctx->delta_key_n, key_n, sizeof(key_n));
    ctx->delta_valid = 1;
    return SEGK_OK;
}

// K1: matrix waves (top-2 values per row and range) + hint waves (the hinted component in reference arithmetic).  One launch
// with both parameter sets, the larger of their grids and LDS sizes.
template <int KS>
static int launch_k1(segk_ctx *ctx, const ScoreArgs &A, const int32_t *remap, int64_t n_emb, const HintLaunch &L, const DeltaBuf &B,
                     int delta_cap, hipStream_t st)
{
    constexpr int TL = KS * 256 + 32;
    HintArgs H{};
    H.ximg = (const unsigned char *)A.X32;
    H.ids = A.ids; H.row0 = A.row0; H.n = A.n;
    H.K_max = A.K_max;
    H.dbg = segk_dev_env("SEGK_HINT_DBG");
#ifdef SEGK_STAMP
    H.stamp = getenv("SEGK_STAMP_PTR") ? (unsigned long long *)strtoull(getenv("SEGK_STAMP_PTR"), nullptr, 0) : nullptr;
#endif
    H.fb_w = L.fb_w; H.fb_t = L.fb_t; H.fb_cur = L.fb_cur;
    H.remap = remap;
    // queue lengths of the call (the caller's ambiguity queue, deferred by segk_kmeans_score_hinted, and the second stage's)
    H.zero_cnt = ctx->defer_zero;
    ctx->defer_zero = nullptr;
    H.pre_hdr = ctx->pre_queue;
    H.k1_groups = L.k1_groups;
    H.xrows32 = A.xrows32; H.ld32 = A.ld32; H.means32 = A.means32;
    H.cand_k = A.cand.k;
    H.nxx = A.xerr + n_emb;                                      // -|x|^2 per row, behind the residual norms
    H.hint_out = L.hint_out;
    H.ctl = B.ctl; H.meanchg = B.meanchg; H.snap_img = B.snap_img;
    H.full = K1Set{A.tiles + 1024, A.n_tiles, L.lds.tpr, L.lds.n_ranges, (float2 *)ctx->hint_part, L.grid};
    size_t lds = (size_t)L.lds.tpr * TL * sizeof(float) + L.lds.map_bytes;
    int grid = L.grid;
    if (B.ctl) {
        // one range over the packed image, every workgroup's slots over all rows
        const int64_t steps = (A.n + 64 * SEGK_K1_NW - 1) / (64 * SEGK_K1_NW);
        H.delta = K1Set{B.packed, 0, delta_cap, 1, B.part, (int64_t)ctx->n_cu > steps ? (int)steps : ctx->n_cu};
        const size_t lds_d = (size_t)delta_cap * TL * sizeof(float) + L.lds.map_bytes;
        if (H.delta.grid > grid) grid = H.delta.grid;
        if (lds_d > lds) lds = lds_d;
    }
    const bool prof = segk_prof_now(ctx);
    const int slot = ctx->prof_n % SEGK_PROF_SLOTS;
#define SEGK_K1_LAUNCH(VV)                                                                                                  \
    do {                                                                                                                     \
        SEGK_CHECK_HIP(segk_dyn_lds((const void *)k_kmeans_top2_rs<KS, VV>, lds));                                           \
        if (prof) SEGK_CHECK_HIP(hipEventRecord(ctx->prof_ev[slot][0], st));                                                 \
        hipLaunchKernelGGL((k_kmeans_top2_rs<KS, VV>), dim3((unsigned)grid), dim3(128 * SEGK_K1_NW), lds, st, H);            \
    } while (0)
    switch ((16 * KS - A.D) / 4) {
        case 0: SEGK_K1_LAUNCH(0); break;
        case 1: SEGK_K1_LAUNCH(1); break;
        case 2: SEGK_K1_LAUNCH(2); break;
        default: SEGK_K1_LAUNCH(3); break;
    }
#undef SEGK_K1_LAUNCH
    if (prof) {
        SEGK_CHECK_HIP(hipEventRecord(ctx->prof_ev[slot][1], st));
        ctx->prof_rows[slot] = A.n;
        ctx->prof_kind = 5;
        ctx->prof_launches = 1;
        ctx->prof_n++;
    }
    return SEGK_OK;
}

// K2: the certificate, one thread per row
static void launch_merge(segk_ctx *ctx, const ScoreArgs &A, const HintLaunch &L, const DeltaBuf &B, int ks, hipStream_t st)
{
    HintMergeArgs E{};
    E.part = (const float2 *)ctx->hint_part;
    E.hint_out = L.hint_out;
    E.n_ranges = L.lds.n_ranges;
    E.tiles_hdr = A.tiles;
    E.ximg = (const unsigned char *)A.X32;
    E.ctl = B.ctl;
    E.part_delta = B.part;
    E.lab_base = B.lab_base;
    E.colchg = B.colchg;
    E.meanchg = B.meanchg;
    E.lab_last = B.lab_last;
    E.stats_host = ctx->delta_host_dev;
    // one workgroup per CU, each a contiguous run of at most SEGK_MERGE_ROWS rows
    int64_t grid = (int64_t)ctx->n_cu;
    if (grid * SEGK_MERGE_THREADS > A.n) grid = (A.n + SEGK_MERGE_THREADS - 1) / SEGK_MERGE_THREADS;
    if (grid * SEGK_MERGE_ROWS < A.n) grid = (A.n + SEGK_MERGE_ROWS - 1) / SEGK_MERGE_ROWS;
    const int64_t per = (A.n + grid - 1) / grid;
    hipLaunchKernelGGL(k_hint_merge, dim3((unsigned)grid), dim3(SEGK_MERGE_THREADS), 0, st, A, E, ks * 16, per,
                       L.band ? ctx->pre_thr : nullptr, L.k1_groups * 64);
}

template <int KS>
static int launch_score_hint(segk_ctx *ctx, ScoreArgs A, const int32_t *remap, const int32_t *K_dev, int64_t n_emb, hipStream_t st)
{
    HintLaunch L{};
    L.band = segk_band_applies(A);
    SEGK_REQUIRE(segk_hint_plan(A.K_max, KS, A.n_tiles, &L.lds),
                 "hinted score path: K_max too large for K1's LDS (the label map beside four ranges of tile images at most)");
    if (int rc = hint_workspaces(ctx, A, L, st)) return rc;
    hint_plan_rows(ctx, A, L);
    DeltaBuf B;
    int delta_cap;
    if (int rc = launch_delta_prep<KS>(ctx, A, remap, K_dev, n_emb, L, st, &B, &delta_cap)) return rc;
    if (int rc = launch_k1<KS>(ctx, A, remap, n_emb, L, B, delta_cap, st)) return rc;
    launch_merge(ctx, A, L, B, KS, st);
    // ---- the rows the certificate could not decide: candidates inside the band of the filter's maximum, scored in the
    // reference's arithmetic (segk_score_band.hip); tables beyond its reach keep the three-product second stage
    // (with delta state the band stage records its winners in lab_last, for the next call's carry-over)
    if (L.band) return segk_launch_band(ctx, A, ctx->pre_thr, A.n, B.lab_last, KS, st);
    // ---- the rows K2 queued: all three products (the pre-filter's second stage); its own undecided rows go to cand.queue
    ScoreArgs B2 = A;
    B2.ids = A.pre_queue;
    B2.row0 = 0;
    B2.n = A.n;
    B2.n_dev = ctx->pre_queue;
    if (int rc = segk_launch_sp_second(ctx, B2, KS, st)) return rc;
    SEGK_LAUNCH_CHECK();
    return SEGK_OK;
}

int segk_dispatch_score_hint(segk_ctx *ctx, const ScoreArgs &A, const int32_t *remap, const int32_t *K_dev, int64_t n_emb, int ks, hipStream_t st)
{
    switch (ks) {
        case 1: return launch_score_hint<1>(ctx, A, remap, K_dev, n_emb, st);
        case 2: return launch_score_hint<2>(ctx, A, remap, K_dev, n_emb, st);
        case 3: return launch_score_hint<3>(ctx, A, remap, K_dev, n_emb, st);
        case 4: return launch_score_hint<4>(ctx, A, remap, K_dev, n_emb, st);
        case 5: return launch_score_hint<5>(ctx, A, remap, K_dev, n_emb, st);
        case 6: return launch_score_hint<6>(ctx, A, remap, K_dev, n_emb, st);
        case 7: return launch_score_hint<7>(ctx, A, remap, K_dev, n_emb, st);
        case 8: return launch_score_hint<8>(ctx, A, remap, K_dev, n_emb, st);
        default: break;
    }
    segk_set_error("hinted score path: D out of range");
    return SEGK_ERR_UNSUPPORTED;
}
