// Lab (experiments builds only, tiles 68-71; no tuning table routes them): conv_wstat_f32 with its USOT_WSTAT_* timing switches,
// its kTiles row macro and its launch.  Included by conv_igemm.hip under USOT_EXPERIMENTS, behind TileCfg.
//
// wstat ("weight-stationary"): the big-K convolutions of the batch-1 frame with the FILTERS IN REGISTERS.
//
// What a v3 k-step waits for (round 5; scripts/ablate_kstep.py on Conf_Fusion's conv, 32 x 64 tile, two workgroups per CU):
// whole kernel 115 us; without the filter tile's global loads 111, without its LDS stores 109, WITHOUT THE CONSUMERS' TWO
// FILTER-FRAGMENT ds_read_b128 PER ROUND 77, with no filter traffic at all 67 (= the MFMA time of 10.3 GFLOP at 2.4 GHz).
// Neither deeper fragment prefetch (PF = 2) nor conflict-free XOR-swizzled rows (docs/LAB_NOTEBOOK.md A.3) nor filters fetched straight from global
// memory (ws tiles) recover it: a consumer wave runs at the matrix pipe's rate only with ONE operand fragment read per
// 8 MFMAs.  Filters are constants, so they can stay where the MFMA reads them:
//   * a workgroup = 8 wavefronts (two per SIMD, all of them loaders AND consumers, 512 threads, one workgroup per CU) owns
//     32 output channels for a RANGE of 32-pixel tiles; wave j keeps the A fragments of those 32 channels for the k-rounds
//     j, j + 8, j + 16, ... (a round = 16 k) - K / 128 rounds x 2 channel blocks x 4 registers = 144 VGPRs at K = 2304 -
//     fetched ONCE per workgroup from the fragment-order bank (usot_conv_pack_wfrag_f32), every wave-load 1 KiB contiguous;
//   * the activation operand streams through LDS in panels of 32 pixels x 128 k (one round per wave and panel; 16 KB, three
//     stages, global -> registers -> LDS by all 512 threads two panels ahead, one barrier per panel): per panel a wave reads
//     TWO B fragments and issues 16 MFMAs (2 pixel blocks x 2 channel blocks x 4) - one read per 8 MFMAs;
//   * k is split over the eight waves INSIDE the workgroup: at the end of a pixel tile the eight partial 32 x 32 tiles meet
//     in LDS (32 KB; written before the panel's barrier, summed in wave order 0..7 by waves 0-3 - one 16 x 16 block each -
//     which add bias / residual / activation and store 16 bytes per lane) while the panel stream of the next tile is
//     already in flight.  Accumulation: a wave's chain is K / 8 products (288 at K = 2304, flushed into a running total
//     every four panels = 64 products like every other fp32 conv kernel), then 8 partials in fixed order.
// Per CU and panel: 16 KB from L2 for 2 x 1 024 MFMA cycles per SIMD (v3: 48 KB), filters never re-read.  Needs
// Cin % 128 == 0 (a panel lies inside one filter tap), K == NST * 128 * RPS, Cout % 32 == 0.
#pragma once

namespace {

template <int RPS>
struct WstatGeom {
    static constexpr int BM = 32, BN = 32, PK = 128 * RPS, LDP = PK + 4, STAGE = BM * LDP;      // PK: k per panel
    static constexpr int NSTG = 4;                // LDS stages: panel q + 1 is complete while panel q is multiplied
    static constexpr int threads = 512, lds_bytes = NSTG * STAGE * 4 + 8 * 4 * 64 * 16;          // + the reduction [8 waves][4 blocks][64 lanes] f32x4
};
template <int NST, int RPS, bool BLOCKED = false>
__global__ __launch_bounds__((WstatGeom<RPS>::threads)) void conv_wstat_f32(const ConvBatch bt)
{
    int pi = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q)
        if (q < bt.n && (int)blockIdx.x >= bt.start[q]) pi = q;
    const ConvK &p = bt.p[pi];
    const int bid0 = (int)blockIdx.x - bt.start[pi];
    using Geo = WstatGeom<RPS>;
    constexpr int BM = Geo::BM, PK = Geo::PK, LDP = Geo::LDP;      // PK: k per panel
    constexpr int CPR = PK / 4;                   // 16-byte chunks per panel row
    constexpr int RPP = 512 / CPR;                // rows per pass of the 512 loader threads
    constexpr int XI = BM / RPP;
    constexpr int STAGE = Geo::STAGE, NSTG = Geo::NSTG;
    static_assert(BM % RPP == 0, "loader passes");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *red = smem + NSTG * STAGE;             // [8 waves][4 blocks][64 lanes] f32x4

    // the problem's fields in registers (p is a dynamically indexed reference into the kernel arguments: every use would be an s_load)
    const int pM = p.M, pP = p.P, pOW = p.OW, pH = p.H, pW = p.W, pCin = p.Cin, pKW = p.KW;
    const int pstride = p.stride, ppad_h = p.pad_h, ppad_w = p.pad_w, pdil_h = p.dil_h, pdil_w = p.dil_w;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, quad = lane >> 4;
    const int units = p.groups * p.NT * p.pr;
    const int u = xcd_remap(bid0, units);
    const int pr = u % p.pr, gc = u / p.pr;
    const int cg = gc % p.NT, g = gc / p.NT;
    const int tile0 = (int)((long)p.MT * pr / p.pr), tile1 = (int)((long)p.MT * (pr + 1) / p.pr);
    const int ntile = tile1 - tile0;
    if (ntile <= 0) return;
    const int npan = ntile * NST;
    const int KT = p.K / 64;

    // ---- loader state (runs three panels ahead of the MFMAs); 32-bit element offsets (the launcher checks the map's size)
    const float *__restrict__ xg = p.x + (long)g * p.x_gs;
    const int lr = tid / CPR, kc = tid % CPR;
    int x_ih0[XI], x_iw0[XI], x_nb[XI];
    unsigned xo[XI];                              // BYTE offset of the row's source at the current tap; 0xffffffff: padding / past M
    // Loads go through a buffer descriptor over this group's input map: an offset past its end returns ZEROS, so padding taps and
    // the pixels past M need no select on the loaded data and no second pointer; the channel offset of the panel rides in the
    // instruction's scalar offset - a panel's two loads per thread cost no vector ALU instruction at all
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void *)xg, 0, (int)((long)p.N * pH * pW * pCin * 4), 0x00020000);
    int l_tile = tile0, l_s = 0, l_tap = 0, l_cc = 0;
    auto set_tile = [&](int tile) {
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            const int m = tile * BM + lr + RPP * i;
            const bool ok = m < pM;
            const int mm = ok ? m : 0;
            const int n = mm / pP, pix = mm - n * pP;
            const int oh = pix / pOW, ow = pix - oh * pOW;
            x_ih0[i] = ok ? oh * pstride - ppad_h : -(1 << 20);      // far outside: every tap fails the bounds test
            x_iw0[i] = ow * pstride - ppad_w;
            x_nb[i] = n * pH * pW * pCin + kc * 4;
        }
    };
    auto set_tap = [&](int tap) {
        const int kh = tap / pKW, kw = tap - kh * pKW;
        const int dh = kh * pdil_h, dw = kw * pdil_w;
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            const int ih = x_ih0[i] + dh, iw = x_iw0[i] + dw;
            const bool in = (unsigned)ih < (unsigned)pH && (unsigned)iw < (unsigned)pW;
            xo[i] = in ? (unsigned)(x_nb[i] + (ih * pW + iw) * pCin) * 4u : 0xffffffffu;
        }
    };
    set_tile(l_tile);
    set_tap(0);
    f32x4 xr[2][XI];
    int l_left = npan;                                       // panels not yet fetched
    auto load_issue = [&](auto dc) {
        constexpr int d = decltype(dc)::value;
#pragma unroll
        for (int i = 0; i < XI; ++i)
#if defined(USOT_WSTAT_LOADSAME)     // timing: every panel fetches the SAME lines (L1 hits: the issue side of the loads alone)
            xr[d][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, (int)(kc * 16 + i * 4096 + lr * 512), 0, 0));
#elif defined(USOT_WSTAT_LOADHALF)   // timing: half the bytes (both loads of a thread fetch its first row)
            xr[d][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, (int)xo[0], l_cc * 4, 0));
#else
            xr[d][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, (int)xo[i], l_cc * 4, 0));
#endif
    };
    auto load_advance = [&]() {
        // wave-uniform counters: kept in scalar registers (readfirstlane: hipcc otherwise carries them in VGPRs under exec masks)
        l_left = __builtin_amdgcn_readfirstlane(l_left - 1);
        if (l_left > 0) {                   // past the last panel the state stops advancing (the panel is fetched again, never stored)
            l_cc = __builtin_amdgcn_readfirstlane(l_cc + PK);
            l_s = __builtin_amdgcn_readfirstlane(l_s + 1);
            if (l_s == NST) {
                l_s = 0; l_cc = 0; l_tap = 0;
                l_tile = __builtin_amdgcn_readfirstlane(l_tile + 1);
                set_tile(l_tile);
                set_tap(0);
            } else if (l_cc == pCin) {
                l_cc = 0;
                l_tap = __builtin_amdgcn_readfirstlane(l_tap + 1);
                set_tap(l_tap);
            }
        }
    };
    auto load_next = [&](auto dc) { load_issue(dc); load_advance(); };
    auto store_panel = [&](auto dc, int st) {
        constexpr int d = decltype(dc)::value;
        float *sX = smem + st * STAGE;
#ifdef USOT_WSTAT_NOWAIT        // timing: the fetched panel is never waited for (the stores write other registers)
#pragma unroll
        for (int i = 0; i < XI; ++i) *(f32x4 *)(sX + (lr + RPP * i) * LDP + kc * 4) = f32x4{1.f * lr, 2.f, 3.f * d, 4.f};
#else
#pragma unroll
        for (int i = 0; i < XI; ++i) *(f32x4 *)(sX + (lr + RPP * i) * LDP + kc * 4) = xr[d][i];
#endif
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    // panels 0 and 1 go to LDS before the first barrier, panel 2 waits in register buffer 0, panel 3 in buffer 1
    load_next(I0{});
    load_next(I1{});

    // ---- this wave's filter fragments: rounds (s * 8 + wave) * RPS + rr of the 32 channels [cg * 32, cg * 32 + 32)
    f32x4 wb[NST][RPS][2];
    {
        const float *wbase = p.w + (long)g * p.w_gs + lane * 4;
#pragma unroll
        for (int s = 0; s < NST; ++s)
#pragma unroll
            for (int rr = 0; rr < RPS; ++rr) {
                const int R = (s * 8 + wave) * RPS + rr;
#pragma unroll
                for (int tn = 0; tn < 2; ++tn)
                    wb[s][rr][tn] = *(const f32x4 *)(wbase + (((long)(cg * 2 + tn) * KT + (R >> 2)) * 4 + (R & 3)) * 256);
            }
    }
    store_panel(I0{}, 0);
    load_next(I0{});
    if (npan > 1) store_panel(I1{}, 1);
    load_next(I1{});
    __syncthreads();

    f32x4 acc[2][2];
    BlockTotal tot[BLOCKED ? 2 : 1][BLOCKED ? 2 : 1];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int tm = 0; tm < 2; ++tm) {
            acc[tn][tm] = zero;
            if constexpr (BLOCKED) tot[tn][tm].clear();
        }
    constexpr int FLUSH = RPS == 1 ? 4 : 2;       // BLOCKED: panels per 64-product block of a wave's chain
    const int fx_off = l15 * LDP + wave * RPS * 16 + quad * 4;
    // gap (0..3 = after MFMA group 0..2, 3 = before group 0) in which this wave stores / fetches: the store of buffer d must
    // precede the fetch into buffer d within a panel, so st_gap comes first in the order 3, 0, 1, 2
    const int wsl = __builtin_amdgcn_readfirstlane(wave & 3);
    const int st_gap = (wsl == 0 || wsl == 3) ? 3 : wsl - 1;  // program order of the gaps: 3, 0, 1, 2
    const int ld_gap = wsl == 3 ? 2 : wsl;
    f32x4 fx[2][RPS][2];                          // [slot][round][pixel block]: slot q & 1 holds panel q's B fragments
    auto read_x = [&](auto sl, int st) {
        constexpr int slot = decltype(sl)::value;
        const float *sX = smem + st * STAGE + fx_off;
#pragma unroll
        for (int rr = 0; rr < RPS; ++rr)
#pragma unroll
            for (int tm = 0; tm < 2; ++tm) fx[slot][rr][tm] = *(const f32x4 *)(sX + tm * 16 * LDP + rr * 16);
    };
    read_x(I0{}, 0);

    int q = 0, st = 0;                            // panel index, its LDS stage
    auto panel = [&](auto sc, auto dc, int tile) {
        constexpr int s = decltype(sc)::value;
        constexpr int d = decltype(dc)::value;    // q & 1: fragment slot of panel q, register buffer of panel q + 2 (stored now) and q + 4 (fetched now)
        const int st1 = (st + 1) & 3, st2 = (st + 2) & 3;
        // panel q + 1 has been complete in its stage since the previous barrier: its fragments travel while this panel is multiplied
#ifndef USOT_WSTAT_NOREAD
        if (q + 1 < npan) read_x(std::integral_constant<int, 1 - d>{}, st1);
#endif
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (BLOCKED && s % FLUSH == 0 && s > 0) {
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                for (int tm = 0; tm < 2; ++tm) tot[tn][tm].add(acc[tn][tm]);
        }
        // A wave issues in order and an MFMA waits for the pipe (32 cycles each, 64 with the SIMD's other wave): everything else
        // of the panel - the LDS store of panel q + 2, the fetch of panel q + 4, the loader's index arithmetic - is placed BETWEEN
        // the four k-slot groups of the panel's MFMAs (pinned: hipcc otherwise issues the 16 MFMAs first and the rest behind them,
        // where both waves of a SIMD sit in the same phase and the matrix pipe idles: 1 920 vs 1 024 cycles per panel)
        auto mma4 = [&](auto cc, int rr) {
            constexpr int c = decltype(cc)::value;
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                for (int tm = 0; tm < 2; ++tm)
                    acc[tn][tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[s][rr][tn][c], fx[d][rr][tm][c],
                                                                       (((BLOCKED && s % FLUSH == 0) || s == 0) && rr == 0 && c == 0) ? zero : acc[tn][tm], 0, 0, 0);
        };
        using C0 = std::integral_constant<int, 0>; using C1 = std::integral_constant<int, 1>;
        using C2 = std::integral_constant<int, 2>; using C3 = std::integral_constant<int, 3>;
        // ... and STAGGERED over the waves: all eight run the same panel between the same two barriers, and eight fetches (or eight
        // LDS stores) issued at the same point queue up in one unit while every wave's MFMA stream waits behind its own
        // instruction; wave w fetches in gap (w & 3) and stores in gap ((w + 2) & 3) of the panel's four MFMA groups
        auto gap = [&](int g4) {
            __builtin_amdgcn_sched_barrier(0);
#ifndef USOT_WSTAT_NOSTORE
            // panel q + 2 (fetched two panels ago) -> its stage (held panel q - 2, whose last reader passed two barriers ago)
            if (g4 == st_gap && q + 2 < npan) store_panel(dc, st2);
#endif
#ifndef USOT_WSTAT_NOLOAD
            if (g4 == ld_gap) load_issue(dc);                 // panel q + 4 (after the store of the same buffer: gaps are cyclic)
#endif
            __builtin_amdgcn_sched_barrier(0);
        };
        static_assert(RPS == 1, "the gap schedule below is written for one round per panel");
        gap(3);                                               // cyclic order of a buffer's uses: store (gap st) ... fetch (gap ld) ...
        mma4(C0{}, 0);
        gap(0);
        mma4(C1{}, 0);
        gap(1);
        mma4(C2{}, 0);
        gap(2);
        load_advance();
        __builtin_amdgcn_sched_barrier(0);
        mma4(C3{}, 0);
        if constexpr (s == NST - 1) {             // the tile's partial sums meet in LDS (read after this panel's barrier)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                for (int tm = 0; tm < 2; ++tm) {
                    f32x4 v = acc[tn][tm];
                    if constexpr (BLOCKED) { tot[tn][tm].add(v); v = tot[tn][tm].get(); tot[tn][tm].clear(); }
                    *(f32x4 *)(red + ((wave * 4 + tn * 2 + tm) * 64 + lane) * 4) = v;
                }
        }
        st = st1;
        ++q;
#ifndef USOT_WSTAT_NOBAR       // timing builds (results are garbage): no per-panel barrier / no panel stores / no panel loads / no fragment reads
        __syncthreads();
#endif
        if constexpr (s == NST - 1) {
            if (wave < 4) {                       // wave w: block (tn, tm) = (w >> 1, w & 1), the eight partials in wave order
                const int tn = wave >> 1, tm = wave & 1;
                f32x4 v = zero;
#pragma unroll
                for (int j = 0; j < 8; ++j) v += *(const f32x4 *)(red + ((j * 4 + wave) * 64 + lane) * 4);
                const int m = tile * BM + tm * 16 + l15;
                const int co = cg * 32 + tn * 16 + quad * 4;
                if (m < p.M) {
                    const float *__restrict__ bg = p.bias ? p.bias + (long)g * p.b_gs : nullptr;
                    const float *__restrict__ rg = p.res ? p.res + (long)g * p.r_gs : nullptr;
                    float *__restrict__ yg = p.y + (long)g * p.y_gs;
                    if (p.vec_store) {
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
    };
#ifdef USOT_WSTAT_NOWAIT
#define USOT_WSTAT_SINK() do { _Pragma("unroll") for (int i = 0; i < XI; ++i) { asm volatile("" :: "v"(xr[0][i])); asm volatile("" :: "v"(xr[1][i])); } } while (0)
#else
#define USOT_WSTAT_SINK()
#endif
    for (int tile = tile0; tile < tile1; ++tile) {
        const bool flip = (NST & 1) && ((tile - tile0) & 1);       // odd panel counts: the buffer parity flips from tile to tile
        if (!flip) {
            [&]<int... Is>(std::integer_sequence<int, Is...>) {
                (panel(std::integral_constant<int, Is>{}, std::integral_constant<int, Is & 1>{}, tile), ...);
            }(std::make_integer_sequence<int, NST>{});
        } else {
            [&]<int... Is>(std::integer_sequence<int, Is...>) {
                (panel(std::integral_constant<int, Is>{}, std::integral_constant<int, (Is + 1) & 1>{}, tile), ...);
            }(std::make_integer_sequence<int, NST>{});
        }
    }
    USOT_WSTAT_SINK();
}

#define TILES(nst, rps, blocked) { F_WSTAT, "conv_wstat_f32<NST=" #nst ",RPS=" #rps ">", WstatGeom<rps>::BM, WstatGeom<rps>::BN, 64, 1, GEOM(WstatGeom<rps>), 1, false, nst, rps, conv_wstat_f32<nst, rps, blocked>, nullptr }

// the launcher's F_WSTAT branch: one workgroup per (group, 32 channels, pixel range); usot_dv = the current device's slot
int launch_wstat(const TileCfg &tc, int tile, void *stream, const usot_conv_desc *d, int n, ConvBatch &bt, int usot_dv)
{
    long blocks = 0;
    double work = 0;
    for (int i = 0; i < n; ++i) work += (double)bt.p[i].M * bt.p[i].Cout * bt.p[i].groups;
    int cus = 256;
    {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
            cus = prop.multiProcessorCount;
    }
    for (int i = 0; i < n; ++i) {
        ConvK &p = bt.p[i];
        const int pk = 128 * tc.rps;
        if (p.K != tc.nst * pk || (d[i].Cin % pk) || (d[i].Cout & 31) || p.ksplit != 1 || d[i].w_frag != 1) return USOT_EINVAL;
        if (p.groups > 1 && (p.w_gs % ((long)16 * p.K))) return USOT_EINVAL;
        if ((long)p.N * p.H * p.W * p.Cin >= (1L << 31)) return USOT_EINVAL;        // 32-bit element offsets in the loader
        p.MT = (p.M + 31) / 32;
        p.NT = d[i].Cout / 32;
        // pixel ranges: this problem's share of the CUs (one workgroup per CU: 8 waves x ~220 VGPRs), by its share of the work
        const double share = (double)p.M * p.Cout * p.groups / work;
        int pr = (int)(cus * share / ((double)p.groups * p.NT));
        if (d[i].ksplit < 0) pr = -d[i].ksplit;            // experiments: ksplit = -PR forces the number of pixel ranges
        p.pr = pr < 1 ? 1 : (pr > p.MT ? p.MT : pr);
        bt.start[i] = (int)blocks;
        blocks += (long)p.groups * p.NT * p.pr;
    }
    for (int i = n; i < 5; ++i) bt.start[i] = (int)blocks;
    static bool raised_d[USOT_MAX_DEV][128] = {};
    bool (&raised)[128] = raised_d[usot_dv];
    if (!raised[tile]) {
        if (hipFuncSetAttribute((const void *)tc.fn, hipFuncAttributeMaxDynamicSharedMemorySize, tc.lds_bytes) != hipSuccess)
            return USOT_ELAUNCH;
        raised[tile] = true;
    }
    hipLaunchKernelGGL(tc.fn, dim3((unsigned)blocks), dim3(tc.threads), tc.lds_bytes, (hipStream_t)stream, bt);
    if (hipGetLastError() != hipSuccess) return USOT_ELAUNCH;
    return USOT_OK;
}

}  // namespace
