// Lab (experiments builds only, tiles 72-78; no tuning table routes them): conv_igemm_f32_v3p with SkInfo, sk_plan, its kTiles
// row macro and its launch.  Included by conv_igemm.hip under USOT_EXPERIMENTS, behind conv_f32_v3.h and TileCfg.
//
// v3p: v3 as a PERSISTENT stream-K launch (whole-chip rounds).
//
// The launch's work is the list of (tile, k-tile) UNITS of all its problems - N-strip-major, so that a contiguous range of units
// is one filter strip x consecutive pixel tiles.  G resident workgroups (one or two per CU, never more than fit) each take
// a contiguous share of U / G units (XCD x takes the x-th eighth of the list: one filter strip per L2) and walk it SEGMENT by
// segment (a segment = the part of one tile inside the share).  A segment that covers its tile's whole k range ends in v3's
// epilogue.  A partial segment stores the wave's accumulators - in register order, 1 KiB per store, write-through (sc1) - to the
// tile's slab [part][wave][block][lane], drains, and takes a ticket PER CONSUMER WAVE; the wave that finds the other parts
// already there (the last to arrive) reads them back, adds them IN PART ORDER (= k order: the same bits whoever is last) and
// runs the epilogue.  No workgroup barrier, no spin, nothing that depends on placement or dispatch order (Guideline 16, recipe
// R1); tickets return to zero.  Producer waves never see any of this: they run ahead into the next segment's first k-tiles
// while the consumers finish the previous one - the launch pays ONE start-up and one drain instead of one per tile, and ends
// within one k-tile of U / G for every workgroup, which is what lets the 64 x 64 tile (2/64 of M N K instead of 3/64 or 4/64
// L2 bytes) be used where 552 tiles over 256 slots would otherwise quantise to three rounds.
#pragma once

namespace {

struct SkInfo {                   // per problem: where its units start and how its tiles are numbered
    int ubase[5];                 // first unit of problem i (ubase[n] = U)
    int tbase[5];                 // first slab / ticket index of problem i
    int G;                        // workgroups of the launch
    int pmax;                     // parts a slab has room for
};

template <int BM, int BN, int NPW, int BK>
struct V3pGeom {
    static constexpr int LD = BK + 4, STAGE = (BM + BN) * LD, lds_bytes = 3 * STAGE * 4;
    static constexpr int threads = 256 + 64 * NPW, min_waves = (BM * BN <= 32 * 64) ? (4 + NPW) / 2 : 1;
};
template <int BM, int BN, int WM, int WN, int D, int NPW, int BK = 64>
__global__ __launch_bounds__((V3pGeom<BM, BN, NPW, BK>::threads), (V3pGeom<BM, BN, NPW, BK>::min_waves)) void conv_igemm_f32_v3p(const ConvBatch bt, const SkInfo sk)
{
    using Geo = V3pGeom<BM, BN, NPW, BK>;
    static_assert(WM * WN == 4, "4 consumer wavefronts");
    constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
    constexpr int LD = Geo::LD, STAGE = Geo::STAGE;
    constexpr int CPR = BK / 4;
    constexpr int NPT = 64 * NPW;
    constexpr int RPP = NPT / CPR;
    constexpr int XI = (BM + RPP - 1) / RPP, WI = (BN + RPP - 1) / RPP;
    constexpr int NR = BK / 16;
    constexpr int NBLK = TM * TN;                 // 16 x 16 blocks of a consumer wave

    extern __shared__ __attribute__((aligned(16))) float smem[];
    const bool producer = threadIdx.x >= 256;
    const int tid = producer ? (int)threadIdx.x - 256 : (int)threadIdx.x;
    const int U = sk.ubase[bt.n];
    // XCD x (blocks b with b % 8 == x) walks the x-th contiguous eighth of the unit list
    const int wi = xcd_remap((int)blockIdx.x, sk.G);
    const int u_begin = (int)((long)U * wi / sk.G), u_end = (int)((long)U * (wi + 1) / sk.G);
    auto owner = [&](long u) { return (int)(((u + 1) * sk.G - 1) / U); };      // index (wi) of the workgroup whose share holds unit u

    auto each_buffer = [&](auto f) {
        [&]<int... Is>(std::integer_sequence<int, Is...>) { (f(std::integral_constant<int, Is>{}), ...); }(std::make_integer_sequence<int, D>{});
    };

    int u = u_begin;
    while (u < u_end) {
        // ---- decode the segment [u, u1): problem, tile, k range (wave-uniform; both wave kinds compute the same)
        int pi = 0;
#pragma unroll
        for (int q = 1; q < 4; ++q)
            if (q < bt.n && u >= sk.ubase[q]) pi = q;
        const ConvK &p = bt.p[pi];
        const int KT = p.K / BK;
        const int cch = p.Cin / BK;
        const int local = u - sk.ubase[pi];
        const int tl = local / KT, kt0 = local - tl * KT;            // tile of the problem (groups x N-strips x M-tiles), first k-tile
        const int ut0 = sk.ubase[pi] + tl * KT;                       // the tile's first unit
        const int u1 = min(u_end, ut0 + KT);
        const int nt = u1 - u;
        const int tiles = p.MT * p.NT;
        const int g = tl / tiles, t0 = tl - g * tiles;
        const int bn0 = (t0 / p.MT) * BN, bm0 = (t0 % p.MT) * BM;
        u = u1;

        if (producer) {
            const float *__restrict__ xg = p.x + (long)g * p.x_gs;
            const float *__restrict__ wg = p.w + (long)g * p.w_gs;
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
            const float *wp[WI];
#pragma unroll
            for (int i = 0; i < WI; ++i) {
                const int row = lr + RPP * i;
                const int co = bn0 + row;
                wp[i] = wg + (long)((row < BN && co < p.Cout) ? co : 0) * p.K + kc * 4 + (long)kt0 * BK;
            }
            f32x4 xr[D][XI], wr[D][WI];
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
                for (int i = 0; i < XI; ++i) {
                    xr[d][i] = *(const f32x4 *)(xin[i] ? xp[i] + c0 : xg + kc * 4);
                    xz[d][i] = xin[i];
                }
#pragma unroll
                for (int i = 0; i < WI; ++i) {
                    wr[d][i] = *(const f32x4 *)wp[i];
                    wp[i] += advance ? BK : 0;
                }
                if (advance && ++cur_cc == cch) {
                    cur_cc = 0;
                    set_tap(++cur_tap);
                }
            };
            auto store_tile = [&](auto dc, int st) {
                constexpr int d = decltype(dc)::value;
                float *sX = smem + st * STAGE, *sW = sX + BM * LD;
#pragma unroll
                for (int i = 0; i < XI; ++i)
                    if (BM % RPP == 0 || lr + RPP * i < BM)
                        *(f32x4 *)(sX + (lr + RPP * i) * LD + kc * 4) = xz[d][i] ? xr[d][i] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < WI; ++i)
                    if (BN % RPP == 0 || lr + RPP * i < BN) *(f32x4 *)(sW + (lr + RPP * i) * LD + kc * 4) = wr[d][i];
            };
            using I0 = std::integral_constant<int, 0>;
            using I1 = std::integral_constant<int, D >= 2 ? 1 : 0>;
            int lt = 0;
            auto load_next = [&](auto dc) { load_tile(dc, lt + 1 < nt); ++lt; };
            // the previous segment's last barrier has passed: every consumer has finished reading every stage
            load_next(I0{});
            load_next(I1{});
            store_tile(I0{}, 0);
            if (nt > 1) store_tile(I1{}, 1);
            each_buffer([&](auto dc) { load_next(dc); });
            __syncthreads();
            int st2 = 2;
            auto step = [&](auto dc, int t) {
                if (t + 2 < nt) store_tile(dc, st2);
                load_next(dc);
                st2 = st2 == 2 ? 0 : st2 + 1;
                __syncthreads();
            };
            int t = 0;
            for (; t + D <= nt; t += D) each_buffer([&](auto dc) { step(dc, t + decltype(dc)::value); });
            each_buffer([&](auto dc) {
                if (t < nt) { step(dc, t); ++t; }
            });
            continue;                                   // next segment: its loads are issued while the consumers finish this one
        }

        // ---------------- consumers
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
        f32x4 acc2 = {0.f, 0.f, 0.f, 0.f};
        BlockTotal tot[TN][TM];
#pragma unroll
        for (int i = 0; i < TN; ++i)
#pragma unroll
            for (int j = 0; j < TM; ++j) { acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; tot[i][j].clear(); }
        auto flush = [&]() {
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j) tot[i][j].add(acc[i][j]);
            if constexpr (TM * TN == 1) tot[0][0].add(acc2);
        };
        const bool whole = nt == KT;                     // the segment IS the tile: v3's epilogue
        // bias and residual travel while the producers bring the first k-tiles (whole tiles, vectorised stores)
        const bool pre = p.vec_store && whole;
        f32x4 pb[TN], pr[TN][TM];
#pragma unroll
        for (int i = 0; i < TN; ++i) {
            const int co = bn0 + (wn * TN + i) * 16 + quad * 4;
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
        __syncthreads();
        read_frags(0, 0, 0);
        int st = 0;
        for (int t = 0; t < nt; ++t) {
            const int st1 = st == 2 ? 0 : st + 1;
            flush();
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                if (r + 1 < NR) read_frags(st, r + 1, (r + 1) & 1);
                else if (t + 1 < nt) read_frags(st1, 0, 0);
                blocked_mma<TN, TM>(acc, acc2, fw[r & 1], fx[r & 1], r == 0);
            }
            st = st1;
            __syncthreads();
        }
        flush();
#pragma unroll
        for (int i = 0; i < TN; ++i)
#pragma unroll
            for (int j = 0; j < TM; ++j) acc[i][j] = tot[i][j].get();

        if (!whole) {
            // ---- partial tile: this wave's blocks -> slab [tile][part][wave][block][lane]; one ticket per (tile, wave)
            const int w_first = owner(ut0), w_last = owner((long)ut0 + KT - 1);
            const int nparts = w_last - w_first + 1, part = wi - w_first;
            const long tslot = sk.tbase[pi] + tl;
            float *slab = p.ws + (tslot * sk.pmax) * (long)(BM * BN);
            int *tick = (int *)(p.ws + (long)sk.tbase[bt.n] * sk.pmax * (BM * BN)) + tslot * 4 + wave;
            const long ntot = (long)sk.tbase[bt.n] * sk.pmax * (BM * BN) * 4;
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)p.ws, 0, (int)(ntot > 0x7fffffffL ? 0x7fffffffL : ntot), 0x00020000);
            auto off = [&](int prt, int blk) { return (int)((((tslot * sk.pmax + prt) * 4 + wave) * NBLK + blk) * 64 + lane) * 16; };
            (void)slab;
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j)
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, acc[i][j]), rs, off(part, i * TM + j), 0, 16);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            int ticket = 0;
            if (lane == 0) ticket = __hip_atomic_fetch_add(tick, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ticket = __builtin_amdgcn_readfirstlane(ticket);
            if (ticket != nparts - 1) continue;           // another part's wave finishes this wave-tile
            if (lane == 0) __hip_atomic_store(tick, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // sum the parts in order (this wave's own part from the slab too: the same bits whichever wave is last)
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j) {
                    f32x4 v = {0.f, 0.f, 0.f, 0.f};
                    for (int q = 0; q < nparts; ++q)
                        v += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off(q, i * TM + j), 0, 16));
                    acc[i][j] = v;
                }
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
                    if (whole) {
                        v += pb[i] + pr[i][j];
                    } else {
                        if (bg) v += *(const f32x4 *)(bg + co);
                        if (rg) v += *(const f32x4 *)(rg + (long)m * p.res_cstride + p.res_coff + co);
                    }
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
}

#define TILEP(bm, bn, wm, wn, d, npw, bk) { F_V3P, "conv_igemm_f32_v3p<" #bm "," #bn ",BK=" #bk ",D=" #d ",NPW=" #npw ">", bm, bn, bk, 1, GEOM(V3pGeom<bm, bn, npw, bk>), 0, false, 0, 0, nullptr, conv_igemm_f32_v3p<bm, bn, wm, wn, d, npw, bk> }

// geometry of a persistent stream-K launch of `n` problems on tile tc (id `tile`): fills bt.p[i].MT/NT, sk; returns the workspace floats
// (slabs [tile][part][BM x BN] + four ticket words per tile) or a negative status
int64_t sk_plan(const TileCfg &tc, int tile, const usot_conv_desc *d, int n, ConvBatch &bt, SkInfo &sk)
{
    long U = 0, T = 0;
    int ktmax = 1;
    for (int i = 0; i < n; ++i) {
        ConvK &p = bt.p[i];
        if (d[i].Cin % tc.bk || p.ksplit != 1 || d[i].w_frag || d[i].defer) return USOT_EINVAL;
        p.MT = (p.M + tc.bm - 1) / tc.bm;
        p.NT = (d[i].Cout + tc.bn - 1) / tc.bn;
        const int kt = p.K / tc.bk;
        sk.ubase[i] = (int)U;
        sk.tbase[i] = (int)T;
        U += (long)p.groups * p.MT * p.NT * kt;
        T += (long)p.groups * p.MT * p.NT;
        ktmax = kt > ktmax ? kt : ktmax;
    }
    if (U <= 0 || U > 0x3fffffffL) return USOT_EINVAL;
    for (int i = n; i < 5; ++i) { sk.ubase[i] = (int)U; sk.tbase[i] = (int)T; }
    const int usot_dv = usot_device_slot();
    if (usot_dv < 0) return USOT_ESTATE;
    static int slots_d[USOT_MAX_DEV][128] = {};
    int (&slots)[128] = slots_d[usot_dv];                       // resident workgroups of this tile on the current device
    if (!slots[tile]) {
        if (hipFuncSetAttribute((const void *)tc.skfn, hipFuncAttributeMaxDynamicSharedMemorySize, tc.lds_bytes) != hipSuccess) return USOT_ELAUNCH;
        int dev = 0, cus = 256, occ = 1;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void *)tc.skfn, tc.threads, tc.lds_bytes) != hipSuccess || occ < 1) occ = 1;
        slots[tile] = cus * (occ > 2 ? 2 : occ);
    }
    long G = slots[tile];
    if (G > U / 4) G = U / 4 > 0 ? U / 4 : 1;          // at least four k-tiles per workgroup
    sk.G = (int)G;
    const long share = U / G;                          // the smallest share
    sk.pmax = (int)((ktmax + share - 1) / share) + 1;  // a tile of KT units meets at most ceil(KT / share) + 1 shares
    const int64_t fl = (int64_t)T * sk.pmax * tc.bm * tc.bn + (int64_t)T * 4;
    if ((int64_t)T * sk.pmax * tc.bm * tc.bn * 4 >= 0x7fffffffLL) return USOT_EINVAL;
    return fl;
}

// the launcher's F_V3P branch: a resident set of workgroups shares the (tile, k-tile) units
int launch_streamk(const TileCfg &tc, int tile, void *stream, const usot_conv_desc *d, int n, ConvBatch &bt)
{
    SkInfo sk;
    const int64_t need = sk_plan(tc, tile, d, n, bt, sk);
    if (need < 0) return (int)need;
    if (!d[0].ws) return USOT_EINVAL;
    for (int i = 0; i < n; ++i) bt.p[i].ws = d[0].ws;         // one workspace for the batch
    for (int i = 0; i < 5; ++i) bt.start[i] = 0;
    hipLaunchKernelGGL(tc.skfn, dim3((unsigned)sk.G), dim3(tc.threads), tc.lds_bytes, (hipStream_t)stream, bt, sk);
    if (hipGetLastError() != hipSuccess) return USOT_ELAUNCH;
    return USOT_OK;
}

}  // namespace
