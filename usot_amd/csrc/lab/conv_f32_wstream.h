// Lab (experiments builds only, tiles 61-65; no tuning table routes them): conv_igemm_f32_ws with its USOT_WS_* timing switches
// and its kTiles row macro; the launcher's general path launches it (w_frag = 1).  Included by conv_igemm.hip under USOT_EXPERIMENTS.
//
// ws ("weight-streaming"): v3's producer / consumer split with the FILTER operand taken out of LDS.
//
// Measured on v3 (scripts/ablate_kstep.py, -DUSOT_ABL_NOW: the W operand neither loaded, staged nor read; 32 x 64 tile):
// Conf_Fusion's conv 112.8 -> 66.8 us (= the MFMA time of its 10.3 GFLOP at 2.4 GHz), one tower level 28.4 -> 18.3,
// layer3's 3x3 27.7 -> 18.0 — two thirds of a k-step's LDS traffic (16 of 24 KB written, 32 of 48 KB read) and two thirds
// of the producers' instructions are the filter tile, and that traffic, not the matrix pipe, is what a CU runs out of
// (two workgroups per CU are only 1.12 x faster than one).  Filters are constants: the host stores them in MFMA FRAGMENT
// order (usot_conv_pack_wfrag: [channel block of 16][k-tile of 64][round of 16 k][lane][4 floats], a permutation
// inside every 16-row block, so row offsets that are multiples of 16 and group strides keep their values) and each
// consumer wave fetches the A fragments of ITS 16 channels straight from global memory into registers, DW k-tiles
// ahead: one fully coalesced 1-KiB global_load_dwordx4 per round, no LDS, no second reader — the four consumer waves
// split the CHANNELS of the tile (wave w: channels 16 w TN ... ), every wave multiplies all BM pixels.  The activation
// tile keeps v3's path (producer waves, global -> registers -> LDS, three stages, one barrier per k-tile); a consumer
// reads TM = BM / 16 B fragments per round for TM x TN MFMA blocks.  All W loads are unconditional and the k-loop is
// unrolled over the DW register buffers, so the compiler counts vmcnt exactly (nothing else of a consumer's loop is
// a vector-memory instruction).
#pragma once

namespace {

template <int BM, int NPW>
struct WsGeom {      // BK = 64; three stages of the activation operand only
    static constexpr int LD = 64, STAGE = BM * LD, threads = 256 + 64 * NPW, lds_bytes = 3 * STAGE * 4;
};
template <int BM, int BN, int D, int NPW, int DW, int WM = 1>
__global__ __launch_bounds__((WsGeom<BM, NPW>::threads)) void conv_igemm_f32_ws(const ConvBatch bt)
{
    int pi = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q)
        if (q < bt.n && (int)blockIdx.x >= bt.start[q]) pi = q;
    const ConvK &p = bt.p[pi];
    const int bid0 = (int)blockIdx.x - bt.start[pi];
    constexpr int BK = 64;
    constexpr int WN = 4 / WM;                    // consumer waves: WM along the pixels x WN along the channels
    constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
    static_assert(TM >= 1 && TN >= 1 && BM % (16 * WM) == 0 && BN % (16 * WN) == 0, "four consumer waves split the tile");
    using Geo = WsGeom<BM, NPW>;
    constexpr int LD = Geo::LD, STAGE = Geo::STAGE;      // unpadded rows, 16-byte chunk c of row `row` stored at chunk c ^ (row & 15): conflict-free fragment reads
    constexpr int CPR = BK / 4;
    constexpr int NPT = 64 * NPW;
    constexpr int RPP = NPT / CPR;
    constexpr int XI = (BM + RPP - 1) / RPP;
    constexpr int NR = BK / 16;
    static_assert(RPP % 16 == 0, "a producer thread's rows share row & 15");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    const bool producer = threadIdx.x >= 256;
    const int tid = producer ? (int)threadIdx.x - 256 : (int)threadIdx.x;
    const int tiles = p.MT * p.NT;
    const int total = tiles * p.groups * p.ksplit;
    const int b = xcd_remap(bid0, total);
    const int z = b / tiles, t0 = b - z * tiles;
    const int g = z / p.ksplit, ks = z - g * p.ksplit;
    const int bn0 = (t0 / p.MT) * BN, bm0 = (t0 % p.MT) * BM;
    const int KT = p.K / BK;
    const int cch = p.Cin / BK;
    const int kt0 = (int)((long)KT * ks / p.ksplit);
    const int kt1 = (int)((long)KT * (ks + 1) / p.ksplit);
    const int nt = kt1 - kt0;

    auto each_of = [&]<int... Is>(std::integer_sequence<int, Is...>, auto f) { (f(std::integral_constant<int, Is>{}), ...); };

    if (producer) {
        const float *__restrict__ xg = p.x + (long)g * p.x_gs;
        const int lr = tid / CPR, kc = tid % CPR;
        int x_ih0[XI], x_iw0[XI];
        long x_nb[XI];
        bool x_ok[XI];
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            const int row = lr + RPP * i;
            const int m = bm0 + row;
            x_ok[i] = (row < BM) && (m < p.M);
            const int mm = x_ok[i] ? m : 0;
            const int n = mm / p.P, pix = mm - n * p.P;
            const int oh = pix / p.OW, ow = pix - oh * p.OW;
            x_ih0[i] = oh * p.stride - p.pad_h;
            x_iw0[i] = ow * p.stride - p.pad_w;
            x_nb[i] = (long)n * p.H * p.W * p.Cin + kc * 4;
        }
        f32x4 xr[D][XI];
        bool xz[D][XI];
        const float *xp[XI];
        bool xin[XI];
        int cur_tap = kt0 / cch, cur_cc = kt0 - cur_tap * cch;
        auto set_tap = [&](int tap) {
            const int kh = tap / p.KW, kw = tap - kh * p.KW;
            const int dh = kh * p.dil_h, dw = kw * p.dil_w;
#pragma unroll
            for (int i = 0; i < XI; ++i) {
                const int ih = x_ih0[i] + dh, iw = x_iw0[i] + dw;
                xin[i] = x_ok[i] && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
                xp[i] = xg + x_nb[i] + ((long)ih * p.W + iw) * p.Cin;
            }
        };
        set_tap(cur_tap);
        auto load_tile = [&](auto dc, bool advance) {
            constexpr int d = decltype(dc)::value;
            const int c0 = cur_cc * BK;
#pragma unroll
            for (int i = 0; i < XI; ++i) {      // unconditional (see v3): padding taps read pixel 0 and are zeroed at the LDS store
                xr[d][i] = *(const f32x4 *)(xin[i] ? xp[i] + c0 : xg + kc * 4);
                xz[d][i] = xin[i];
            }
            if (advance && ++cur_cc == cch) {
                cur_cc = 0;
                set_tap(++cur_tap);
            }
        };
        auto store_tile = [&](auto dc, int st) {
            constexpr int d = decltype(dc)::value;
            float *sX = smem + st * STAGE;
            const int kcs = (kc ^ (lr & 15)) * 4;
#pragma unroll
            for (int i = 0; i < XI; ++i)
                if (BM % RPP == 0 || lr + RPP * i < BM)
                    *(f32x4 *)(sX + (lr + RPP * i) * LD + kcs) = xz[d][i] ? xr[d][i] : f32x4{0.f, 0.f, 0.f, 0.f};
        };
        using I0 = std::integral_constant<int, 0>;
        using I1 = std::integral_constant<int, D >= 2 ? 1 : 0>;
        int lt = 0;
        auto load_next = [&](auto dc) { load_tile(dc, lt + 1 < nt); ++lt; };
        if constexpr (D == 1) {
            load_next(I0{}); store_tile(I0{}, 0);
            load_next(I0{}); if (nt > 1) store_tile(I0{}, 1);
        } else {
            load_next(I0{});
            load_next(I1{});
            store_tile(I0{}, 0);
            if (nt > 1) store_tile(I1{}, 1);
        }
        each_of(std::make_integer_sequence<int, D>{}, [&](auto dc) { load_next(dc); });
        __syncthreads();
        int st2 = 2;
        auto step = [&](auto dc, int t) {
            if (t + 2 < nt) store_tile(dc, st2);
            load_next(dc);
            st2 = st2 == 2 ? 0 : st2 + 1;
            __syncthreads();
        };
        int t = 0;
        for (; t + D <= nt; t += D) each_of(std::make_integer_sequence<int, D>{}, [&](auto dc) { step(dc, t + decltype(dc)::value); });
        each_of(std::make_integer_sequence<int, D>{}, [&](auto dc) {
            if (t < nt) { step(dc, t); ++t; }
        });
        return;
    }

    // ---------------- consumers: wave w owns channels bn0 + 16 TN w ... of all BM pixels
    const int lane = tid & 63, wave = (tid >> 6) / WM, wm = (tid >> 6) % WM;
    const int l15 = lane & 15, quad = lane >> 4;
    const int fx_off = (wm * TM * 16 + l15) * LD;
    const int swz = (quad ^ l15) * 4;
    // fragment-order filter stream of this wave's channel blocks (blocks past the padded bank read block 0: never stored)
    const int ncb = (p.Cout + 15) >> 4;
    const float *wq[TN];
#pragma unroll
    for (int i = 0; i < TN; ++i) {
        const int cb = (bn0 >> 4) + wave * TN + i;
        wq[i] = p.w + (long)g * p.w_gs + ((long)(cb < ncb ? cb : 0) * KT + kt0) * (BK * 16) + lane * 4;
    }
    f32x4 wb[DW][TN][NR];
    f32x4 fx[2][TM];
    auto read_x = [&](int st, int r, int slot) {
        const float *base = smem + st * STAGE + ((r * 16) ^ swz) + fx_off;
#pragma unroll
        for (int j = 0; j < TM; ++j) fx[slot][j] = *(const f32x4 *)(base + j * 16 * LD);
    };
    f32x4 acc[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 acc2 = {0.f, 0.f, 0.f, 0.f};
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
    // bias and residual first (v3: fetched while the first k-tiles travel), THEN the filter stream: vector loads return in
    // order, so the wait for the first filter fragments covers them
    const bool pre = p.vec_store && p.ksplit == 1;
    f32x4 pb[TN], pr[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; ++i) {
        const int co = bn0 + (wave * TN + i) * 16 + quad * 4;
        const bool cok = pre && co + 3 < p.Cout;
        pb[i] = (cok && p.bias) ? *(const f32x4 *)(p.bias + (long)g * p.b_gs + co) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < TM; ++j) {
            const int m = bm0 + (wm * TM + j) * 16 + l15;
            pr[i][j] = (cok && p.res && m < p.M)
                           ? *(const f32x4 *)(p.res + (long)g * p.r_gs + (long)m * p.res_cstride + p.res_coff + co)
                           : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
#ifdef USOT_WS_NOWAIT
    f32x4 sink[DW][TN][NR];
#endif
    int lt = 0;
    auto wnext = [&](auto dc) {                      // fetch the next k-tile of the stream into buffer dc (past the end: the last tile again)
        constexpr int d = decltype(dc)::value;
        const bool advance = lt + 1 < nt;
#pragma unroll
        for (int i = 0; i < TN; ++i) {
#pragma unroll
            for (int r = 0; r < NR; ++r) {
#if defined(USOT_WS_NOWLOAD)          // timing builds (scripts/ablate_kstep.py): the filter stream never issued ...
                wb[d][i][r] = f32x4{1.f + r, 2.f, 3.f, 4.f + d};
#elif defined(USOT_WS_NOWAIT)         // ... or issued but never waited for inside the loop (MFMAs on constants)
                sink[d][i][r] = *(const f32x4 *)(wq[i] + r * 256);
                wb[d][i][r] = f32x4{1.f + r, 2.f, 3.f, 4.f + d};
#else
                wb[d][i][r] = *(const f32x4 *)(wq[i] + r * 256);
#endif
            }
            wq[i] += advance ? BK * 16 : 0;
        }
        ++lt;
    };
    each_of(std::make_integer_sequence<int, DW>{}, [&](auto dc) { wnext(dc); });
    __syncthreads();
    if (nt > 0) read_x(0, 0, 0);
    int st = 0;
    auto step = [&](auto dc, int t) {
        constexpr int d = decltype(dc)::value;
        const int st1 = st == 2 ? 0 : st + 1;
        flush();
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            if (r + 1 < NR) read_x(st, r + 1, (r + 1) & 1);
            else if (t + 1 < nt) read_x(st1, 0, 0);
#ifndef USOT_WS_NOPIN
            // the NEXT round's B fragments leave LDS while this round's MFMAs issue; unpinned, hipcc sinks the reads below the
            // MFMAs, right in front of their first use, and every round then waits a full LDS latency (k-step 1 620 vs 1 040 cycles)
            __builtin_amdgcn_sched_barrier(0);
#endif
            f32x4 wfr[TN];
#pragma unroll
            for (int i = 0; i < TN; ++i) wfr[i] = wb[d][i][r];
            blocked_mma<TN, TM>(acc, acc2, wfr, fx[r & 1], r == 0);
        }
        wnext(dc);
        st = st1;
        __syncthreads();
    };
    {
        int t = 0;
        for (; t + DW <= nt; t += DW) each_of(std::make_integer_sequence<int, DW>{}, [&](auto dc) { step(dc, t + decltype(dc)::value); });
        each_of(std::make_integer_sequence<int, DW>{}, [&](auto dc) {
            if (t < nt) { step(dc, t); ++t; }
        });
    }
    flush();
#ifdef USOT_WS_NOWAIT
#pragma unroll
    for (int d = 0; d < DW; ++d)
#pragma unroll
        for (int i = 0; i < TN; ++i)
#pragma unroll
            for (int r = 0; r < NR; ++r) asm volatile("" :: "v"(sink[d][i][r]));
#endif
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = tot[i][j].get();

    if (p.ksplit > 1) {
#pragma unroll
        for (int j = 0; j < TM; ++j) {
            const int m = bm0 + (wm * TM + j) * 16 + l15;
            if (m >= p.M) continue;
#pragma unroll
            for (int i = 0; i < TN; ++i) {
                const int co = bn0 + (wave * TN + i) * 16 + quad * 4;
                const long el = ((long)(ks * p.groups + g) * p.M + m) * p.Cout + co;
                if (co + 3 < p.Cout && (p.Cout & 3) == 0) {
                    ws_store4(p, el, acc[i][j]);
                } else {
                    for (int e = 0; e < 4; ++e)
                        if (co + e < p.Cout) ws_store1(p, el + e, acc[i][j][e]);
                }
            }
        }
        if (p.combine) splitk_combine<BM, BN>(p, g, t0, tiles, bm0, bn0, tid, (int *)smem);
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
            const int co = bn0 + (wave * TN + i) * 16 + quad * 4;
            if (co >= p.Cout) continue;
            f32x4 v = acc[i][j];
            if (p.vec_store && co + 3 < p.Cout) {
                v += pb[i] + pr[i][j];
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
                    float s2 = v[e];
                    if (bg) s2 += bg[c];
                    if (rg) s2 += rg[(long)m * p.res_cstride + p.res_coff + c];
                    s2 = apply_act(s2, c < p.act_split ? p.act : p.act2);
                    if (p.y_nchw) yg[((long)n * p.Cout + c) * p.P + pix] = s2;
                    else          yg[(long)m * p.y_cstride + p.y_coff + c] = s2;
                }
            }
        }
    }
}

#define TILEW(bm, bn, d, npw, dw, wm) { F_WS, "conv_igemm_f32_ws<" #bm "," #bn ",D=" #d ",NPW=" #npw ",DW=" #dw ">", bm, bn, 64, 1, GEOM(WsGeom<bm, npw>), 1, false, 0, 0, conv_igemm_f32_ws<bm, bn, d, npw, dw, wm>, nullptr }

}  // namespace
