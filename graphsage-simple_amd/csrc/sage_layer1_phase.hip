// Layer 1 of the gcn encoder in ONE launch on the slice-major table, phase-sliced:
//     h1[r] = act1( mean_j table[nbr1[r, j]] . W1^T )
// without the [|S1|, D0] means ever leaving the chip (the split form writes them with the column-sliced gather and reads them back in
// the contraction: two launches, 24 MB out and 24 MB in at BASELINE config 3).
//
// What the split form's gather owes its speed to is that an XCD's private L2 holds ONE 128-byte slice of the hot rows.  The one-launch
// layers of sage_fused.hip gather whole rows and lose that.  Here the slicing is kept in TIME instead of in space:
//   * a block owns TILES of 32 destination rows (tile t goes to block t mod grid; the grid is a multiple of 8, blocks are dealt round
//     robin over the 8 XCDs, so XCD x owns the tiles of class x: an eighth of the rows whatever the device-side row count is);
//   * it walks the D0 / 32 slices of the table in PHASES.  In a phase it gathers slice p of its 32 rows exactly as the rows form of the
//     sliced gather does (sage_gather_body.h: lane group of 8 lanes x 16 B per (row, slice), every neighbour in flight, sum in list
//     order), so at any time an XCD's L2 is asked for one slice of an eighth of the rows;
//   * the 32 x 32 slice means go to LDS as the three bf16 planes of the exact split (sage_split_bf16.h) and are contracted with the
//     phase's 32 columns of the prepared W1 planes (sage_prepare_weights' register order, 24 KiB per phase, L2-resident) by six
//     v_mfma_f32_32x32x16_bf16 per 16 k.  The accumulators of the tile (32 rows x H1, wave w = columns [32 w, 32 w + 32)) stay in
//     registers over all phases: K is split in time, there are no partial sums in memory.
// Bits.  Every phase order and every accumulator is that of the split form: slices in ascending order for every block (NOT rotated by
// XCD: a row's bits must not depend on the tile, block or XCD it lands on, and fp32 accumulation is order dependent), K half 0 (the
// first half of the slices) and K half 1 in two accumulators of the same wave that meet as half 0 + half 1, the MFMA order of
// dense_bf16x3_kernel inside a step, the gather's sums in list order.  The result equals gather + contraction BIT FOR BIT
// (tests/test_gpu_layer1_fused.py), so the two forms can be mixed freely (training keeps the means, serving does not).
// Rows that hold |x| >= 2^127 / Inf / NaN in their means (the empty-set NaN rule included), or every row when W1 holds one, are
// recomputed by the exact fp32 fma chain of the contraction's cold path, from the table.
// Latency: in the one-tile form 3 blocks of 4 waves per CU take turns -- while one contracts and stages, the others have their 16 x 1 KiB per
// wave in flight.  The pair form (below, the default: SAGE_L1P_TILES) keeps rows in flight inside the wave instead.
#include "sage_gather_body.h"
#include "sage_split_bf16.h"

namespace {

using namespace sage_split_detail;
using sage_gather_detail::gather_rows_unit_add;
using sage_gather_detail::gather_rows_unit_issue;
using sage_gather_detail::gather_rows_unit_mean;
using sage_gather_detail::gather_rows_unit_scale;
using sage_gather_detail::gather_rows_unit_sum;
using sage_gather_detail::gather_v4;

struct PhaseArgs {
    const float* table; int table_rows; int64_t slice_stride;     // slice-major: float[D0 / 32][table_rows][32]
    const int32_t* nbr; const int32_t* cnt; int k;
    int n; const int32_t* n_dev; int n_off;
    const int32_t* self_row; const int32_t* any_nonempty;
    const float* W; int64_t ldw; const uint4* wsplit; int out_dim; int act;
    float* out; int64_t ldo;
};

constexpr int kTileRows = 32;         // destination rows per tile = per MFMA
constexpr int kSliceFloats = 32;      // 128-byte slices: 8 lanes x 16 B
constexpr int kMaxK = SAGE_MAX_FANOUT;
constexpr int kOutLd = 128 + 4;         // floats per row of the output tile in LDS
constexpr int kPlaneLd = kSliceFloats + 8;                    // bf16 elements per LDS row of a plane (+16 B)
constexpr int kPlane = kTileRows * kPlaneLd;                  // one plane of a tile's slice means

// the mean of column kk of row `lr` of the tile, as the vector path computes it (same terms, same order)
__device__ inline float exact_mean(const PhaseArgs& a, const int32_t* ids, int c, int s, bool extra, bool nan_rule, int kk) {
    const int last_row = a.table_rows - 1;
    const float* col = a.table + (int64_t)(kk / kSliceFloats) * a.slice_stride + (kk % kSliceFloats);
    float sum = 0.f;
    for (int j = 0; j < c; ++j) sum += col[(int64_t)min(max(ids[j], 0), last_row) * kSliceFloats];
    if (extra) sum += col[(int64_t)min(s, last_row) * kSliceFloats];
    const int ceff = c + (extra ? 1 : 0);
    if (ceff > 0) return sum * (1.0f / (float)ceff);
    return nan_rule ? __builtin_nanf("") : 0.f;
}

// A phase's 32 columns of the prepared W1 planes for this wave's column group: [K half][column group = wave][step][plane][lane] x 16 B
template <int STEPS>
__device__ __forceinline__ void load_w1_phase(const uint4* wsplit, const int kg, const int q, const int wave, const int lane, bf16x8 (&bw)[2][3]) {
    const uint4* wp = wsplit + ((size_t)(kg * 4 + __builtin_amdgcn_readfirstlane(wave)) * STEPS + 2 * q) * 3 * 64;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) bw[j][pl] = __builtin_bit_cast(bf16x8, wp[(j * 3 + pl) * 64 + lane]);
}

// One slice of one tile: the lane's 4 means of tile row lr -> huge flags, the three planes in `buf` -> block barrier -> the wave's 12 MFMAs
__device__ __forceinline__ f32x16 contract_slice(const gather_v4 res, __bf16* buf, const int lr, const int gl, const int lane, const bool mfma_wave,
                                                 int* rowflag_lr, int* tileflag, const bf16x8 (&bw)[2][3], f32x16 acc) {
    constexpr int LDB = kPlaneLd, PL = kPlane;
    if (huge4(res)) { *rowflag_lr = 1; *tileflag = 1; }              // same value from every writer
    {
        bf16x4 hi, mid, lo;
        split3(res, hi, mid, lo);
        __bf16* dst = buf + lr * LDB + gl * 4;
        *reinterpret_cast<bf16x4*>(dst) = hi;
        *reinterpret_cast<bf16x4*>(dst + PL) = mid;
        *reinterpret_cast<bf16x4*>(dst + 2 * PL) = lo;
    }
    lds_barrier();
    if (mfma_wave) {
        const __bf16* abase = buf + (lane & 31) * LDB + 8 * (lane >> 5);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const bf16x8 ah = *reinterpret_cast<const bf16x8*>(abase + 16 * j);
            const bf16x8 am = *reinterpret_cast<const bf16x8*>(abase + PL + 16 * j);
            const bf16x8 al = *reinterpret_cast<const bf16x8*>(abase + 2 * PL + 16 * j);
            acc = mfma_bf16x3_step(ah, am, al, bw[j], acc);
        }
    }
    return acc;
}

// A tile's epilogue: half 0 + half 1 -> [row][column] tile in LDS -> activation -> whole 512-B rows, streaming stores; then the cold
// path.  ids / cnts / selfs / rowflag / tileflag are the tile's own.  Ends with every thread past its reads of outp only after the next
// block barrier.
template <int NSLICE>
__device__ __forceinline__ void tile_epilogue(const PhaseArgs& a, const int tile, const int nn, const f32x16 (&acc)[2], float* outp,
                                              const int32_t* ids, const int32_t* cnts, const int32_t* selfs, const int* rowflag,
                                              const int* tileflag, const bool w_huge, const bool nan_rule) {
    constexpr int M = kTileRows, PLD = kOutLd;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i32 = lane & 31, h = lane >> 5, n0 = wave * 32, k = a.k;
    if (n0 < a.out_dim) {
        float* mine = outp + n0 + i32;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) mine[((reg & 3) + 8 * (reg >> 2) + 4 * h) * PLD] = acc[0][reg] + acc[1][reg];
    }
    lds_barrier();
    const bool any_bad = *tileflag != 0;
#pragma unroll 1                                          // (unrolled, its addresses are hoisted out of the tile loop and held over the phases)
    for (int it = 0; it < M * 32 / 256; ++it) {
        const int idx = it * 256 + tid;
        const int row = idx >> 5, col = (idx & 31) * 4;
        const int g = tile * M + row;
        if (g < nn && col < a.out_dim && !(any_bad && (w_huge || rowflag[row] != 0))) {      // out_dim % 32 == 0 (host-checked)
            const f32x4 pv = *reinterpret_cast<const f32x4*>(outp + row * PLD + col);
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = sage_activate(pv[e], a.act);
            sage_store_stream<SAGE_H1_STORE>(reinterpret_cast<f32x4*>(a.out + (int64_t)g * a.ldo + col), v);
        }
    }
    // rows with a huge value (all rows when W1 holds one): the exact fp32 fma chain over k, torch.mm's Inf / NaN behaviour.
    // Block-uniform; never taken on ordinary data.
    if (any_bad) {
        const int d0 = NSLICE * kSliceFloats;
        for (int idx = tid; idx < M * a.out_dim; idx += 256) {
            const int row = idx / a.out_dim, col = idx % a.out_dim;
            const int g = tile * M + row;
            if (g >= nn || !(w_huge || rowflag[row] != 0)) continue;
            const int32_t* rid = ids + row * k;
            const int rc = cnts[row], rs = selfs[row];
            bool rextra = rs >= 0;
            for (int j = 0; j < rc; ++j) rextra = rextra && rid[j] != rs;
            const float* wrow = a.W + (int64_t)col * a.ldw;
            float dot = 0.f;
            for (int kk = 0; kk < d0; ++kk) dot = fmaf(exact_mean(a, rid, rc, rs, rextra, nan_rule, kk), wrow[kk], dot);
            a.out[(int64_t)g * a.ldo + col] = sage_activate(dot, a.act);
        }
    }
}

template <int NSLICE>
__global__ __launch_bounds__(256, 3) void layer1_phase_kernel(const PhaseArgs a) {
    constexpr int M = kTileRows, SL = 8, TRIP = 16;
    constexpr int PL = kPlane, PLD = kOutLd;
    constexpr int STEPS = NSLICE;                         // 16-k steps per K half of the prepared planes (KP = 32 NSLICE)
    __shared__ __attribute__((aligned(16))) __bf16 planes[2 * 3 * PL];
    __shared__ __attribute__((aligned(16))) float outp[M * PLD];
    __shared__ int32_t ids[M * kMaxK];
    __shared__ int32_t cnts[M], selfs[M];
    __shared__ int rowflag[M];                            // the row's means hold a huge value (this tile)
    __shared__ int tileflag;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int nn = a.n;
    if (a.n_dev) nn = min(*a.n_dev + a.n_off, a.n);
    const int ntiles = (nn + M - 1) / M;
    const bool nan_rule = a.any_nonempty ? (*a.any_nonempty != 0) : false;
    const int last_row = a.table_rows - 1;
    const int grp = lane / SL, gl = lane % SL;
    const int lr = wave * (kWave / SL) + grp;             // the tile row whose slices this lane group gathers
    const bool mfma_wave = wave * 32 < a.out_dim;
    const int k = a.k;
    const bool w_huge = a.wsplit[(size_t)8 * STEPS * 3 * 64].x != 0;     // the trailer sage_prepare_weights leaves behind the planes

    for (int tile = (int)blockIdx.x; tile < ntiles; tile += (int)gridDim.x) {
        __syncthreads();                                  // the previous tile's ids / flags / output tile have been read
        for (int i = tid; i < M * k; i += 256) {
            const int rq = min(tile * M + i / k, nn - 1); // rows past the end shadow the last row (nothing of theirs is stored)
            ids[i] = a.nbr[(int64_t)rq * k + i % k];
        }
        if (tid < M) {
            const int rq = min(tile * M + tid, nn - 1);
            cnts[tid] = min(a.cnt[rq], k);
            selfs[tid] = a.self_row ? a.self_row[rq] : -1;
            rowflag[tid] = 0;
        }
        if (tid == 0) tileflag = w_huge ? 1 : 0;
        __syncthreads();
        const bool valid = tile * M + lr < nn;
        const int c = cnts[lr], s = selfs[lr];
        const int32_t* myn = ids + lr * k;

        f32x16 acc[2];                                    // K half 0 / K half 1, as the two wave groups of dense_bf16x3_kernel
#pragma unroll
        for (int e = 0; e < 16; ++e) { acc[0][e] = 0.f; acc[1][e] = 0.f; }
#pragma unroll
        for (int kg = 0; kg < 2; ++kg) {
#pragma unroll 1
            for (int q = 0; q < NSLICE / 2; ++q) {
                const int p = kg * (NSLICE / 2) + q;      // the phase = the slice
                const float* tcol = a.table + (int64_t)p * a.slice_stride + gl * 4;
                bool extra = s >= 0;
                const gather_v4 sum = gather_rows_unit_sum<TRIP, false>(tcol, kSliceFloats, myn, c, k, s, last_row, nullptr, extra);
                // requested once the rows have arrived (the planes' 24 registers beside the 64 of the rows in flight spill), in flight
                // while the means are staged
                bf16x8 bw[2][3];
                load_w1_phase<STEPS>(a.wsplit, kg, q, wave, lane, bw);
                gather_v4 res = gather_rows_unit_mean(sum, c, extra, nan_rule);
                if (!valid) res = gather_v4{0.f, 0.f, 0.f, 0.f};
                // one barrier per phase: the planes are double-buffered, and a wave reaches the next phase's barrier only after its
                // MFMAs of this one
                acc[kg] = contract_slice(res, planes + (p & 1) * 3 * kPlane, lr, gl, lane, mfma_wave, &rowflag[lr], &tileflag, bw, acc[kg]);
            }
        }
        tile_epilogue<NSLICE>(a, tile, nn, acc, outp, ids, cnts, selfs, rowflag, &tileflag, w_huge, nan_rule);
    }
}

// The pair form: a block owns the two tiles (2 j, 2 j + 1) of pair j (pair j goes to block j mod grid) and walks them half a phase
// apart, so that one tile's rows are in flight while the other tile is split and contracted -- in the one-tile form a wave has no
// table bytes in flight from its W1 request to its last MFMA, and a second set of rows there costs the third block of the CU.  Here two
// blocks per CU hold what four one-tile blocks would, the phase's W1 planes are fetched once for both tiles, and a launch of up to
// 2 x 2 x kNumCU tiles is resident in one round.
// Registers decide the grain.  Two full 16-row sets beside two tiles' accumulators (64), the W1 planes (24) and the addresses of a
// set being requested spill, so the ping-pong runs on HALF sets of 8 rows: a half of the arriving tile is summed (list order: half 0,
// then half 1, one add per row) and the same half of the other tile is requested in its place, so 8 to 16 requests of a wave are in
// flight at any time and at most 16.  Per phase p:
//     W1(p) requested | A half 0 summed, B half 0 of slice p requested | A half 1 summed, B half 1 requested | A staged, barrier, A's
//     MFMAs | B half 0 summed, A half 0 of slice p + 1 requested | B half 1 summed, A half 1 requested | B staged, barrier, B's MFMAs
// Loads return in order, so W1(p) goes out BEHIND A's rows and IN FRONT OF B's: A's MFMAs wait for W1 with B's 16 requests still out
// (s_waitcnt vmcnt(16)), and B's MFMAs, on the same W1 registers, wait for no load at all while A's next rows are out.
// Each tile has ONE set of planes: between a tile's MFMAs of phase p and its plane writes of phase p + 1 stands the other tile's barrier.
// Lists longer than 16: the first 16 positions are the ones in flight, the others are fetched four at a time where the row is summed
// (list order kept).  That loop, and the self row that rides with half 0, exist only in the instantiations that need them (LONG, SELF).
// Bits: every row's arithmetic is the one-tile form's, term by term; the huge flags are per tile.
// 233 VGPRs (d0 = 256, no self row, k <= 16; at most 250 over the instantiations), no scratch, 49 416 B of LDS, 2 blocks per CU.
template <int NSLICE, bool SELF, bool LONG>
__global__ __launch_bounds__(256, 2) void layer1_pair_kernel(const PhaseArgs a) {
    constexpr int M = kTileRows, SL = 8, HALF = 8;        // HALF: rows per request set, half of the one-tile form's trip
    constexpr int MORE = 4;                               // rows per request of a long list's tail (beside the other tile's sets in flight)
    constexpr int PL = kPlane, PLD = kOutLd;
    constexpr int STEPS = NSLICE;
    __shared__ __attribute__((aligned(16))) __bf16 planes[2 * 3 * PL];     // [tile of the pair][plane]
    __shared__ __attribute__((aligned(16))) float outp[M * PLD];           // the two tiles' epilogues take turns
    __shared__ int32_t ids[2 * M * kMaxK];
    __shared__ int32_t cnts[2 * M], selfs[2 * M];
    __shared__ int rowflag[2 * M];
    __shared__ int tileflag[2];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int nn = a.n;
    if (a.n_dev) nn = min(*a.n_dev + a.n_off, a.n);
    const int npairs = (nn + 2 * M - 1) / (2 * M);
    const bool nan_rule = a.any_nonempty ? (*a.any_nonempty != 0) : false;
    const int last_row = a.table_rows - 1;
    const int grp = lane / SL, gl = lane % SL;
    const int lr = wave * (kWave / SL) + grp;             // the row of either tile whose slices this lane group gathers
    const bool mfma_wave = wave * 32 < a.out_dim;
    const int k = a.k;
    const bool w_huge = a.wsplit[(size_t)8 * STEPS * 3 * 64].x != 0;

    for (int pair = (int)blockIdx.x; pair < npairs; pair += (int)gridDim.x) {
        __syncthreads();                                  // the previous pair's ids / flags / output tile have been read
        {
            const int row = tid >> 2;                     // four threads per row of the pair
            const int rq = min(pair * 2 * M + row, nn - 1);       // rows past the end shadow the last row (nothing of theirs is stored)
            for (int j = tid & 3; j < k; j += 4) ids[row * k + j] = a.nbr[(int64_t)rq * k + j];
        }
        if (tid < 2 * M) {
            const int rq = min(pair * 2 * M + tid, nn - 1);
            cnts[tid] = min(a.cnt[rq], k);
            selfs[tid] = SELF ? a.self_row[rq] : -1;
            rowflag[tid] = 0;
        }
        if (tid < 2) tileflag[tid] = w_huge ? 1 : 0;
        __syncthreads();
        // tile A = 2 pair, tile B = 2 pair + 1; index [0] / [1] below
        bool valid[2], extra[2];
        float scale[2];                                   // 1 / |set|, below zero for the empty set
        int c[2], s[2];
        const int32_t* myn[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            valid[t] = pair * 2 * M + t * M + lr < nn;
            c[t] = cnts[t * M + lr];
            s[t] = selfs[t * M + lr];
            myn[t] = ids + (t * M + lr) * k;
            extra[t] = SELF && s[t] >= 0;                 // the self row joins the set unless it is among the neighbours: the same
            if (SELF)                                     // answer in every phase, so it is found once per pair
                for (int j = 0; j < c[t]; ++j) extra[t] = extra[t] && myn[t][j] != s[t];
            scale[t] = gather_rows_unit_scale(c[t], extra[t]);
        }
        // Half h of a tile's first trip of slice p (list positions [HALF h, HALF h + HALF)), requested; the self row rides with half 0.
        // Nothing waits here.
        auto issue = [&](const int t, const int p, const int h, gather_v4 (&rows)[HALF], gather_v4& selfv) __attribute__((always_inline)) {
            const float* tcol = a.table + (int64_t)p * a.slice_stride + gl * 4;
            bool unused = false;
            // the count read from LDS again, not kept: what is derived from a kept one (a list position per request) is hoisted out of
            // the phase loop, 16 registers per tile that the rows in flight need
            const int cnow = cnts[t * M + lr];
            gather_rows_unit_issue<HALF, false>(tcol, kSliceFloats, myn[t], HALF * h, cnow, k, -1, last_row, nullptr, unused, rows);
            if (SELF && h == 0) selfv = *reinterpret_cast<const gather_v4*>(tcol + (int64_t)min(max(selfs[t * M + lr], 0), last_row) * kSliceFloats);
        };
        // what follows a tile's first trip: the later positions of a long list, the self row, the mean
        auto finish = [&](const int t, const int p, gather_v4 sum, const gather_v4 selfv) __attribute__((always_inline)) {
            const float* tcol = a.table + (int64_t)p * a.slice_stride + gl * 4;
            const int cnow = cnts[t * M + lr];
            for (int j0 = 2 * HALF; LONG && j0 < k; j0 += MORE) {
                gather_v4 more[MORE];
                bool unused = false;
                gather_rows_unit_issue<MORE, false>(tcol, kSliceFloats, myn[t], j0, cnow, k, -1, last_row, nullptr, unused, more);
                gather_rows_unit_add<MORE>(sum, more, j0, cnow);
            }
            if (SELF) {
                const gather_v4 with = sum + selfv;
                if (extra[t]) sum = with;
            }
            gather_v4 res = gather_rows_unit_mean(sum, scale[t], nan_rule);
            if (!valid[t]) res = gather_v4{0.f, 0.f, 0.f, 0.f};
            return res;
        };

        f32x16 acc[2][2];                                 // [tile][K half]
#pragma unroll
        for (int e = 0; e < 16; ++e) { acc[0][0][e] = 0.f; acc[0][1][e] = 0.f; acc[1][0][e] = 0.f; acc[1][1][e] = 0.f; }
        gather_v4 rows_a[2][HALF], self_a = {0.f, 0.f, 0.f, 0.f};
        issue(0, 0, 0, rows_a[0], self_a);
        issue(0, 0, 1, rows_a[1], self_a);
        // last: the launch's last phase requests no further rows of A (a compile-time fork: a run-time one would make the waits for
        // B's rows full ones)
        auto phase = [&](const int kg, const int q, const bool last) __attribute__((always_inline)) {
            const int p = kg * (NSLICE / 2) + q;
            gather_v4 rows_b[2][HALF], self_b = {0.f, 0.f, 0.f, 0.f};
            gather_v4 sum = {0.f, 0.f, 0.f, 0.f};
            // W1(p) is requested BEHIND A's rows and IN FRONT OF B's: loads return in order, so A's MFMAs, which wait for W1, would
            // otherwise wait for B's rows too
            bf16x8 bw[2][3];
            // (the fences keep the scheduler from gathering the requests in front of the sums: the order below IS the register budget)
            load_w1_phase<STEPS>(a.wsplit, kg, q, wave, lane, bw);
            __builtin_amdgcn_sched_barrier(0);
            gather_rows_unit_add<HALF>(sum, rows_a[0], 0, cnts[lr]);
            __builtin_amdgcn_sched_barrier(0);
            issue(1, p, 0, rows_b[0], self_b);
            __builtin_amdgcn_sched_barrier(0);
            gather_rows_unit_add<HALF>(sum, rows_a[1], HALF, cnts[lr]);
            __builtin_amdgcn_sched_barrier(0);
            issue(1, p, 1, rows_b[1], self_b);
            __builtin_amdgcn_sched_barrier(0);
            const gather_v4 res_a = finish(0, p, sum, self_a);
            acc[0][kg] = contract_slice(res_a, planes, lr, gl, lane, mfma_wave, &rowflag[lr], &tileflag[0], bw, acc[0][kg]);
            sum = gather_v4{0.f, 0.f, 0.f, 0.f};
            __builtin_amdgcn_sched_barrier(0);
            gather_rows_unit_add<HALF>(sum, rows_b[0], 0, cnts[M + lr]);
            __builtin_amdgcn_sched_barrier(0);
            if (!last) issue(0, p + 1, 0, rows_a[0], self_a);
            __builtin_amdgcn_sched_barrier(0);
            gather_rows_unit_add<HALF>(sum, rows_b[1], HALF, cnts[M + lr]);
            __builtin_amdgcn_sched_barrier(0);
            if (!last) issue(0, p + 1, 1, rows_a[1], self_a);
            __builtin_amdgcn_sched_barrier(0);
            const gather_v4 res_b = finish(1, p, sum, self_b);
            acc[1][kg] = contract_slice(res_b, planes + 3 * PL, lr, gl, lane, mfma_wave, &rowflag[M + lr], &tileflag[1], bw, acc[1][kg]);
        };
#pragma unroll 1
        for (int q = 0; q < NSLICE / 2; ++q) phase(0, q, false);
#pragma unroll 1
        for (int q = 0; q < NSLICE / 2 - 1; ++q) phase(1, q, false);
        phase(1, NSLICE / 2 - 1, true);

        tile_epilogue<NSLICE>(a, 2 * pair, nn, acc[0], outp, ids, cnts, selfs, rowflag, &tileflag[0], w_huge, nan_rule);
        lds_barrier();                                    // tile A's output tile has been read
        tile_epilogue<NSLICE>(a, 2 * pair + 1, nn, acc[1], outp, ids + M * k, cnts + M, selfs + M, rowflag + M, &tileflag[1], w_huge, nan_rule);
    }
}

template <int NSLICE>
int launch_phase(const PhaseArgs& a, hipStream_t st, sage_launch_events_t* ev) {
    // persistent blocks, a multiple of 8 so that a tile's (a pair's) class mod 8 is its XCD
    const sage_tunables_t& tn = sage_tunables();
    const int per_cu = tn.layer1_phase_per_cu;
    if (tn.layer1_phase_tiles == 2) {
        const int grid = min((sage_cdiv(a.n, 2 * kTileRows) + 7) / 8 * 8, kNumCU * per_cu);
        // SELF: a self row rides with every request set; LONG: lists longer than the two sets in flight (the loop that fetches the rest
        // where the row is summed costs the short lists their partial waits, by its mere presence)
        const bool self = a.self_row != nullptr, lng = a.k > 16;
        if (self && lng) sage_launch(layer1_pair_kernel<NSLICE, true, true>, dim3(grid), dim3(256), 0, st, ev, a);
        else if (self) sage_launch(layer1_pair_kernel<NSLICE, true, false>, dim3(grid), dim3(256), 0, st, ev, a);
        else if (lng) sage_launch(layer1_pair_kernel<NSLICE, false, true>, dim3(grid), dim3(256), 0, st, ev, a);
        else sage_launch(layer1_pair_kernel<NSLICE, false, false>, dim3(grid), dim3(256), 0, st, ev, a);
        SAGE_CHECK_LAUNCH("layer1_pair_kernel");
        return SAGE_OK;
    }
    const int grid = min((sage_cdiv(a.n, kTileRows) + 7) / 8 * 8, kNumCU * per_cu);
    sage_launch(layer1_phase_kernel<NSLICE>, dim3(grid), dim3(256), 0, st, ev, a);
    SAGE_CHECK_LAUNCH("layer1_phase_kernel");
    return SAGE_OK;
}

}  // namespace

bool sage_layer1_phase_supported(int32_t d0, int32_t h1, int32_t k) {
    return (d0 == 64 || d0 == 128 || d0 == 256) && h1 >= 32 && h1 <= 128 && h1 % 32 == 0 && k >= 1 && k <= kMaxK;
}

int sage_launch_layer1_phase(const sage_rows_t& src, const sage_lists_t& l, const sage_contract_t& c, hipStream_t st,
                             sage_launch_events_t* ev) {
    const int32_t d0 = src.dim;
    SAGE_REQUIRE(src.ld == kSliceFloats && src.slice_stride == src.table_rows * (int64_t)kSliceFloats,
                 "layer1_fused: the table must be slice-major with %d-float slices", kSliceFloats);
    if (!sage_layer1_phase_supported(d0, c.out_dim, l.k) || !c.weight_prepared || !sage_aligned(src.table, 16) || !sage_aligned(c.out, 16) ||
        !sage_aligned(c.weight_prepared, 16) || c.ldo % 4 != 0 || c.ldo < c.out_dim || c.ldw < d0) {
        sage_set_error("layer1_fused: unsupported shape d0=%d h1=%d k=%d (or unaligned arrays / no prepared weights)", d0, c.out_dim, l.k);
        return SAGE_EUNSUPPORTED;
    }
    if (l.n == 0) return SAGE_OK;
    const PhaseArgs a{src.table, (int)src.table_rows, src.slice_stride, l.nbr, l.cnt, l.k, l.n, l.n_dev, l.n_off, l.self_row, l.any_nonempty,
                      c.weight, c.ldw, (const uint4*)c.weight_prepared, c.out_dim, c.act, c.out, c.ldo};
    if (d0 == 64) return launch_phase<2>(a, st, ev);
    if (d0 == 128) return launch_phase<4>(a, st, ev);
    return launch_phase<8>(a, st, ev);
}

extern "C" int sage_layer1_fused_supported(int32_t d0, int32_t h1, int32_t k) { return sage_layer1_phase_supported(d0, h1, k) ? 1 : 0; }

extern "C" int sage_layer1_fused(const float* table_sliced, int64_t table_rows, int32_t d0, const int32_t* nbr, const int32_t* cnt,
                                 int32_t k, int32_t n, const int32_t* n_dev, const int32_t* self_row, const int32_t* any_nonempty,
                                 const float* weight, int64_t ldw, const void* weight_prepared, int32_t out_dim, int32_t act, float* out,
                                 int64_t ldo, sage_stream_t stream) {
    SAGE_REQUIRE(table_sliced && nbr && cnt && weight && weight_prepared && out, "layer1_fused: NULL array");
    SAGE_REQUIRE(n >= 0 && table_rows >= 1 && table_rows < (1ll << 31), "layer1_fused: n = %d, table_rows = %lld", n, (long long)table_rows);
    SAGE_REQUIRE(act >= 0 && act <= SAGE_ACT_NONE, "layer1_fused: bad activation");
    return sage_launch_layer1_phase({.table = table_sliced, .table_rows = table_rows, .ld = kSliceFloats, .dim = d0,
                                     .slice_stride = table_rows * (int64_t)kSliceFloats},
                                    {.nbr = nbr, .cnt = cnt, .k = k, .n = n, .n_dev = n_dev, .self_row = self_row, .any_nonempty = any_nonempty},
                                    {.weight = weight, .ldw = ldw, .weight_prepared = weight_prepared, .out_dim = out_dim, .act = act, .out = out,
                                     .ldo = ldo},
                                    (hipStream_t)stream);
}
