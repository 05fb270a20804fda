// v2: conv_igemm_f32_v2.  Main loop: three LDS stages, the barrier in the MIDDLE of a k-tile, fragments
// prefetched one round ahead (also across the k-tile boundary).
//
// At batch 1 most layers run one wavefront per SIMD, so nothing hides a wave's own waits:
// every cycle it spends on ds_write -> barrier -> ds_read -> first MFMA is a cycle the matrix
// pipe idles (measured on v1, 64x64 tile, layer3.0 shortcut: MFMA-only 130 TFLOP/s, with
// staging 58).  Here, per k-tile t:
//     F1 <- fragments(t, round 1)            issued before round 0's MFMAs
//     MFMA round 0 (F0)
//     G (tile t+1, loaded during tile t-1) -> LDS[(t+1)%3];  issue global loads of t+2 -> G
//     barrier                                 (tile t+1 visible; nobody still reads (t+1)%3,
//                                              it held tile t-2)
//     F0 <- fragments(t+1, round 0)          hidden behind round 1's MFMAs
//     MFMA round 1 (F1)
// so the global-load latency has a whole k-tile to land, the LDS write is off the critical
// path, and no MFMA ever waits for a just-issued ds_read.
#pragma once
#include "conv_f32_common.h"

namespace {

template <int BM, int BN, int BK, int KSW>
struct V2Geom {
    static constexpr int LD = BK + 4, STAGE = (BM + BN) * LD;
    static constexpr int threads = 256 * KSW, lds_bytes = KSW * 3 * STAGE * 4;      // three stages per group of four waves
};
template <int BM, int BN, int WM, int WN, int BK, int KSW = 1>
__global__ __launch_bounds__((V2Geom<BM, BN, BK, KSW>::threads)) void conv_igemm_f32_v2(const ConvBatch bt)
{
    // the prologue block of this workgroup's problem in SGPRs (conv_f32_common.h: conv_pro_fetch); `p` stays the way to the fields that
    // are read behind the k-loop only
    int pi, bid0;
    const ConvPro q = conv_pro_fetch(pi, bid0);
    const ConvK &p = bt.p[pi];
    static_assert(WM * WN == 4, "4 wavefronts per workgroup");
    static_assert(BK == 32 || BK == 64, "k-tile of 32 or 64");
    constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
    using Geo = V2Geom<BM, BN, BK, KSW>;
    constexpr int LD = Geo::LD, STAGE = Geo::STAGE;
    constexpr int CPR = BK / 4;                 // 16-byte chunks per row
    constexpr int RPP = 256 / CPR;              // rows covered per pass of the 256 loaders
    constexpr int XI = (BM + RPP - 1) / RPP, WI = (BN + RPP - 1) / RPP;
    constexpr int NR = BK / 16;                 // MFMA rounds per k-tile

    // KSW > 1: the workgroup has KSW groups of 4 wavefronts that share ONE output tile and
    // split its k-tiles round-robin (group g takes kt0+g, kt0+g+KSW, ...), each with its own
    // LDS stages; partial accumulators meet in LDS at the end.  Two (or four) waves per SIMD
    // from the same tile hide each other's staging without a cross-workgroup reduction, a
    // workspace round trip or a second launch (what inter-workgroup split-K costs).
    extern __shared__ __attribute__((aligned(16))) float smem_all[];
    const int grp = KSW > 1 ? (int)(threadIdx.x >> 8) : 0;
    float *smem = smem_all + grp * 3 * STAGE;

    const int tid = threadIdx.x & 255;
    // index prologue: every divisor is a constant of the problem, divided by with its host-made multiplier and shift (fastdiv.h)
    const int tiles = q.tiles;
    const int b = xcd_remap(bid0, q.total);
    const int z = fd_div(b, q.d_tiles), t0 = b - z * tiles;
    const int g = fd_div(z, q.d_ksplit), ks = z - g * q.ksplit;
    const int tn0 = fd_div(t0, q.d_MT);
    const int bn0 = tn0 * BN, bm0 = (t0 - tn0 * q.MT) * BM;
    const int KT = q.ktb;                       // k-tiles of this instantiation
    const int cch = q.cch;
    const int kt0 = fd_div(KT * ks, q.d_ksplit);              // (KT * ksplit < 2^31: the launcher checks)
    const int kt1 = fd_div(KT * (ks + 1), q.d_ksplit);

    const float *__restrict__ xg = q.x + (long)g * q.x_gs;
    const float *__restrict__ wg = q.w + (long)g * q.w_gs;

    const int lr = tid / CPR, kc = tid % CPR;
    int x_ih0[XI], x_iw0[XI];
    long x_nb[XI];
    bool x_ok[XI];
#pragma unroll
    for (int i = 0; i < XI; ++i) {
        const int row = lr + RPP * i;
        const int m = bm0 + row;
        x_ok[i] = (row < BM) && (m < q.M);
        const int mm = x_ok[i] ? m : 0;
        const int n = fd_div(mm, q.d_P), pix = mm - n * q.P;
        const int oh = fd_div(pix, q.d_OW), ow = pix - oh * q.OW;
        x_ih0[i] = oh * q.stride - q.pad_h;
        x_iw0[i] = ow * q.stride - q.pad_w;
        x_nb[i] = (long)n * q.H * q.W * q.Cin + kc * 4;
    }
    long w_off[WI];
    bool w_ok[WI];
#pragma unroll
    for (int i = 0; i < WI; ++i) {
        const int row = lr + RPP * i;
        const int co = bn0 + row;
        w_ok[i] = (row < BN) && (co < q.Cout);
        w_off[i] = (long)(w_ok[i] ? co : 0) * q.K + kc * 4;
    }

    // Loader state is incremental: a row's source pointer is recomputed only when the filter
    // tap changes (every Cin/BK k-tiles, never for a 1x1 conv); inside a tap the next k-tile
    // is just +BK floats.  Keeps the per-k-tile VALU work (exposed at one wave per SIMD) small.
    f32x4 xr[XI], wr[WI];
    const float *xp[XI];
    bool xin[XI];
    const float *wp[WI];
    int cur_tap = fd_div(kt0 + grp, q.d_cch), cur_cc = (kt0 + grp) - cur_tap * cch;
    auto set_tap = [&](int tap) {
        const int kh = fd_div(tap, q.d_KW), kw = tap - kh * q.KW;
        const int dh = kh * q.dil_h, dw = kw * q.dil_w;
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            const int ih = x_ih0[i] + dh, iw = x_iw0[i] + dw;
            xin[i] = x_ok[i] && (unsigned)ih < (unsigned)q.H && (unsigned)iw < (unsigned)q.W;
            xp[i] = xg + x_nb[i] + ((long)ih * q.W + iw) * q.Cin;
        }
    };
    set_tap(cur_tap);
#pragma unroll
    for (int i = 0; i < WI; ++i) wp[i] = wg + w_off[i] + (long)(kt0 + grp) * BK;
    auto load_tile = [&](bool advance) {        // loads the NEXT k-tile in sequence
        const int c0 = cur_cc * BK;
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (xin[i]) v = *(const f32x4 *)(xp[i] + c0);
            xr[i] = v;
        }
#pragma unroll
        for (int i = 0; i < WI; ++i) {
            // rows >= Cout read row 0: they only feed accumulators that are never stored
            wr[i] = *(const f32x4 *)wp[i];
            wp[i] += advance ? KSW * BK : 0;
        }
        if (advance) {
            cur_cc += KSW;
            if (cur_cc >= cch) {
                do { cur_cc -= cch; ++cur_tap; } while (cur_cc >= cch);
                set_tap(cur_tap);
            }
        }
    };
    auto store_tile = [&](int st) {
        float *sX = smem + st * STAGE, *sW = sX + BM * LD;
#pragma unroll
        for (int i = 0; i < XI; ++i)
            if (BM % RPP == 0 || lr + RPP * i < BM) *(f32x4 *)(sX + (lr + RPP * i) * LD + kc * 4) = xr[i];
#pragma unroll
        for (int i = 0; i < WI; ++i)
            if (BN % RPP == 0 || lr + RPP * i < BN) *(f32x4 *)(sW + (lr + RPP * i) * LD + kc * 4) = wr[i];
    };

    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const int l15 = lane & 15, quad = lane >> 4;
    const int fx_off = (wm * TM * 16 + l15) * LD + quad * 4;
    const int fw_off = BM * LD + (wn * TN * 16 + l15) * LD + quad * 4;
    f32x4 fw[2][TN], fx[2][TM];
    auto read_frags = [&](int st, int r, int slot) {
        const float *base = smem + st * STAGE + r * 16;
#pragma unroll
        for (int i = 0; i < TN; ++i) fw[slot][i] = *(const f32x4 *)(base + fw_off + i * 16 * LD);
#pragma unroll
        for (int j = 0; j < TM; ++j) fx[slot][j] = *(const f32x4 *)(base + fx_off + j * 16 * LD);
    };
    f32x4 acc[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // A wave with a single 16x16 block would chain every MFMA on one accumulator (40-cycle
    // dependent latency vs 32-cycle issue: an 80 % cap); it alternates two accumulators instead
    // (even / odd k-slots) and adds them at the end.
    f32x4 acc2 = {0.f, 0.f, 0.f, 0.f};
    // Blocked accumulation (blocked_mma above).  The block boundary sits at the mid-tile barrier: right after it the MFMAs
    // issued before it have retired, the block is added to `tot` and the tile's last round starts the next block with C = 0.
    BlockTotal tot[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) tot[i][j].clear();
    auto flush = [&]() {
#pragma unroll
        for (int i = 0; i < TN; ++i)
#pragma unroll
            for (int j = 0; j < TM; ++j) tot[i][j].add(acc[i][j]);
        if constexpr (TM * TN == 1) tot[0][0].add(acc2);
    };
    auto mma = [&](int slot, bool first) { blocked_mma<TN, TM>(acc, acc2, fw[slot], fx[slot], first); };

    const int nt_all = kt1 - kt0;
    const int nt = (nt_all - grp + KSW - 1) / KSW;      // k-tiles of this wave group
    const int nt_max = (nt_all + KSW - 1) / KSW;        // barriers must match across groups
    if (KSW > 1 && nt <= 0) __syncthreads();
    if (nt > 0) {
        load_tile(nt > 1);
        store_tile(0);
        if (nt > 1) load_tile(nt > 2);
        __syncthreads();
        read_frags(0, 0, 0);
    }
    int st = 0;                                   // stage holding tile t
    for (int t = 0; t < nt_max; ++t) {
        if (KSW > 1 && t >= nt) {                 // this group is out of k-tiles: keep the barrier count
            __syncthreads();
            continue;
        }
        const int st1 = st == 2 ? 0 : st + 1;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            if (r + 1 < NR) read_frags(st, r + 1, (r + 1) & 1);
            if (r == NR - 1) {                     // mid-tile hand-over sits before the LAST round
                if (t + 1 < nt) store_tile(st1);
                if (t + 2 < nt) load_tile(t + 3 < nt);
                __syncthreads();                  // lowers to lgkmcnt(0) + s_barrier (no vmcnt drain)
                if (t + 1 < nt) read_frags(st1, 0, 0);
                flush();
            }
            mma(r & 1, r == NR - 1);
        }
        st = st1;
    }
    flush();
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = tot[i][j].get();

    if (KSW > 1) {
        // meet in LDS: thread (lane, wave) of every group holds the same (channel, pixel) slots
        __syncthreads();
        f32x4 *red = (f32x4 *)smem_all;
        if (grp > 0) {
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j) red[(((grp - 1) * TN + i) * TM + j) * 256 + tid] = acc[i][j];
        }
        __syncthreads();
        if (grp > 0) return;
#pragma unroll
        for (int g2 = 1; g2 < KSW; ++g2)
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j) acc[i][j] += red[(((g2 - 1) * TN + i) * TM + j) * 256 + tid];
    }
    // ---- epilogue (same as v1)
    if (p.ksplit > 1) {
#pragma unroll
        for (int j = 0; j < TM; ++j) {
            const int m = bm0 + (wm * TM + j) * 16 + l15;
            if (m >= p.M) continue;
#pragma unroll
            for (int i = 0; i < TN; ++i) {
                const int co = bn0 + (wn * TN + i) * 16 + quad * 4;
                const long el = ((long)(ks * p.groups + g) * p.M + m) * p.Cout + co;
                if (co + 3 < p.Cout && (p.Cout & 3) == 0) {
                    ws_store4(p, el, acc[i][j]);
                } else {
                    for (int e = 0; e < 4; ++e)
                        if (co + e < p.Cout) ws_store1(p, el + e, acc[i][j][e]);
                }
            }
        }
        if (p.combine) splitk_combine<BM, BN>(p, g, t0, tiles, bm0, bn0, tid, (int *)smem_all);
        return;
    }
    const float *__restrict__ bg = p.bias ? p.bias + (long)g * p.b_gs : nullptr;
    const float *__restrict__ rg = p.res ? p.res + (long)g * p.r_gs : nullptr;
    float *__restrict__ yg = p.y + (long)g * p.y_gs;
#pragma unroll
    for (int j = 0; j < TM; ++j) {
        const int m = bm0 + (wm * TM + j) * 16 + l15;
        if (m >= p.M) continue;
#pragma unroll
        for (int i = 0; i < TN; ++i) {
            const int co = bn0 + (wn * TN + i) * 16 + quad * 4;
            if (co >= p.Cout) continue;
            f32x4 v = acc[i][j];
            if (p.vec_store && co + 3 < p.Cout) {
                if (bg) v += *(const f32x4 *)(bg + co);
                if (rg) v += *(const f32x4 *)(rg + (long)m * p.res_cstride + p.res_coff + co);
                const int a = co < p.act_split ? p.act : p.act2;
                if (a != USOT_ACT_NONE) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = apply_act(v[e], a);
                }
                *(f32x4 *)(yg + (long)m * p.y_cstride + p.y_coff + co) = v;
            } else {
                const int n = m / p.P, pix = m - n * p.P;
                for (int e = 0; e < 4; ++e) {
                    const int c = co + e;
                    if (c >= p.Cout) break;
                    float s = v[e];
                    if (bg) s += bg[c];
                    if (rg) s += rg[(long)m * p.res_cstride + p.res_coff + c];
                    s = apply_act(s, c < p.act_split ? p.act : p.act2);
                    if (p.y_nchw) yg[((long)n * p.Cout + c) * p.P + pix] = s;
                    else          yg[(long)m * p.y_cstride + p.y_coff + c] = s;
                }
            }
        }
    }
}

}  // namespace
