// v3: conv_igemm_f32_v3, the kernel of the batch-1 frame's long reductions, exact fp32 (PF = 1) and split-fp16 (PF = 4, 5).
//
// What is here beside the shipped code, and why.  The default library instantiates WM x WN = 2 x 2 consumer waves, BK = 32 (the 64 x 64
// tile) or 64, D = 1, 2, 3, NPW = 4 or 8 and PF = 1, 4 or 5 (kTiles in conv_igemm.hip: the rows outside XT(...)).  The variants an
// experiments build adds are `if constexpr` branches of THIS kernel and stay here: PF = 2 and PF = 3 (deeper / hand-scheduled fragment
// prefetch), PF = 6 / XDMA (both operands by LDS-DMA), D = 4 and the eight-consumer-wave form (WM x WN = 8).  They have tile ids and
// experiments-build parity tests; lifting them out would mean a second copy of the kernel.  USOT_ABL_* and USOT_TRACE are the
// instruments of scripts/ablate_kstep.py and scripts/trace_kstep.py on the shipped kernel: timing builds only, never defined by
// usot_amd/build.py.  The kernel generations with no routed tile at all (stream-K, weight-streaming, weight-stationary) live in lab/.
//
// Producer / consumer wavefronts.  512 threads: waves 0-3 only feed the matrix pipe
// (ds_read fragments -> MFMA), waves 4-7 only move data (global -> registers -> LDS).
// Each SIMD hosts one of each, so the loader's address math, VMEM issue and LDS writes run in
// the shadow of the other wave's MFMAs instead of inside the MFMA wave's own instruction
// stream — the overlap a one-wave-per-SIMD launch (batch 1) cannot get from occupancy.
// Three LDS stages, one barrier per k-tile; the producers stay two tiles ahead, so at tile t a
// consumer may read tile t and prefetch the first fragments of tile t+1 without waiting:
//     producers, tile t : G (tile t+2) -> stage (t+2)%3 ; issue loads of tile t+3 ; barrier
//     consumers, tile t : rounds of {prefetch next fragments ; MFMAs} ;             barrier
// stage (t+2)%3 held tile t-1, which every consumer finished before barrier(t-1).
// D = k-tiles of global loads a producer keeps in flight in registers: with D = 1 the loads of
// tile t+3 are issued only after those of tile t+2 have landed, so a k-step can never be shorter
// than one L2/HBM round trip (measured: 32x32x64 steps took ~600 ns with the MFMAs removed);
// D = 2/3 rotate that many register buffers so a step only waits for loads issued D steps ago.
// NPW = producer wavefronts (4 or 8): the producers' k-step (four ds_write_b128 + lgkmcnt(0) ~500 cycles, address
// VALU + load issue ~450, measured with s_memtime) is what the consumers wait for; eight producers halve the
// per-wave share.  (Fetching ALL fragments of k-tile t+1 during the MFMAs of tile t, instead of one 16-k round
// ahead, measured 20 % slower and was dropped.)
// (Fetching ALL fragments of k-tile t+1 in front of tile t's MFMAs - pinned with sched_barrier, hipcc otherwise
// sinks the reads to the end of the step - shortens the consumer's MFMA phase 828 -> 712 cycles but the burst of
// ds_read_b128 doubles the producers' ds_write time; k-step 1064 -> 1196.  Not kept.)
// (Unpadded XOR-swizzled rows, staggered producer stores and fragment reads interleaved with the MFMAs were measured and
// refuted: docs/LAB_NOTEBOOK.md A.3.)
// PF = rounds (16 k each) a consumer's fragment reads run ahead of their MFMAs: 1 = two fragment slots; 2 = one slot per round
// of the k-tile (BK = 64), reads issued two rounds = 16 MFMAs ahead and pinned there (sched_barrier)
// PF = 4 (round 5): SPLIT-fp16 arithmetic.  Every fp32 operand is carried as hi + lo, two fp16 numbers (22 significant bits:
// hi = fp16(s v), lo = fp16(s v - hi), s a power of two that puts the tensor near the top of fp16's range), and a product
// w x is formed as w_lo x_hi + w_hi x_lo + w_hi x_hi on v_mfma_f32_16x16x32_f16 with fp32 accumulation - three 16-cycle MFMAs
// per 32 k where the fp32 MFMA needs eight 32-cycle ones (5.3 x less matrix-pipe time), the dropped w_lo x_lo term is 2^-22 of
// the product.  Filters arrive pre-split from the host (engine.py: PackedConv.w_split16 - per output row a power-of-two scale,
// each k-tile of 64 stored as 64 hi halves + 64 lo halves = the 256 bytes of the fp32 row segment, so the producers move them
// unchanged); activations are split by the PRODUCER waves as they stage a tile (x 8, two ds_write_b64 per four values: VALU
// of a sibling wave costs the MFMA waves nothing).  An LDS row is [64 hi | 64 lo]: the consumers' four 16-byte fragment reads
// per row and k-tile are the fp32 kernel's (rounds 0 / 1 = hi of k 0-31 / 32-63, rounds 2 / 3 = lo).  The finished sums are
// multiplied by wscale[co] = 1 / (row scale x 8) (exact: powers of two) before anything else sees them.  Range contract:
// |activation| < 8 188 (fp16 overflow above that shows as inf / nan in the output, never silently); accuracy: within the
// 1e-4 bar of the fp32 path and as close to float64 as it (tests/test_gpu_model.py, tests/golden/f64_gate.py).
#pragma once
#include <type_traits>
#include <utility>
#include "conv_f32_common.h"

namespace {

template <int BM, int BN, int WM, int WN, int BK, int D, int NPW, int PF>
struct V3Geom {
    static constexpr bool H16 = PF == 4 || PF == 5 || PF == 6, XDMA = PF == 6, WDMA = PF == 5 || PF == 6;      // split-fp16 arithmetic (above); activation / filter tile by LDS-DMA
    static constexpr int CT = 64 * WM * WN, NPT = XDMA ? 0 : 64 * NPW;       // consumer threads; the producers follow (none with XDMA)
    static constexpr int NDW = XDMA ? 12 : (WDMA ? 4 : 0);                   // DMA wavefronts, behind the producers
    static constexpr int NSW = WDMA ? ((D >= 4 || PF == 6) ? 6 : 5) : 3, NSX = XDMA ? NSW : 3;      // filter / activation stages
    static constexpr int LD = BK + 4, lds_bytes = (NSX * BM + NSW * BN) * LD * 4;      // rows padded by four floats
    static constexpr int threads = CT + NPT + 64 * NDW;
};
template <int BM, int BN, int WM, int WN, int BK, int D = 1, int NPW = 4, int PF = 1>
__global__ __launch_bounds__((V3Geom<BM, BN, WM, WN, BK, D, NPW, PF>::threads)) void conv_igemm_f32_v3(const ConvBatch bt)
{
    using Geo = V3Geom<BM, BN, WM, WN, BK, D, NPW, PF>;
#ifdef USOT_TRACE
    const unsigned tr_entry = (unsigned)__builtin_readcyclecounter();
#endif
    // the prologue block of this workgroup's problem in SGPRs (conv_f32_common.h: conv_pro_fetch); `p` stays the way to the fields that
    // are read behind the k-loop only
    int pi, bid0;
    const ConvPro q = conv_pro_fetch(pi, bid0);
    const ConvK &p = bt.p[pi];
    // run-time image count (usot_conv_desc.n_dyn): the load is issued first and used behind the index prologue
    // (a scalar fetch through the constant address space: the third and last dependent scalar round of the prologue.  The scalar cache
    // is refreshed at a dispatch boundary only, so the word must be complete before this launch starts: written by an EARLIER kernel
    // or copy of the stream / graph chain, never by anything that may run concurrently with this launch - this kernel itself, a
    // parallel graph branch, another stream or the host)
    const int dyn_n = q.n_dyn ? *(const USOT_KARG int *)(uintptr_t)q.n_dyn : 0;
    // WM x WN consumer wavefronts: 4 (one per SIMD) or 8 (two per SIMD, round 5: the same tile in smaller wave tiles, nothing to
    // exchange).  Probe (scripts/probes/coissue_probe.hip, inline-asm reads, independent accumulators): a SIBLING wave's VALU / SALU /
    // LDS / VMEM instructions do not delay a wave's back-to-back MFMAs at all (32.0 cycles each); the wave's OWN ds_read_b128, issued
    // a round ahead, cost ~6 cycles each (292 / 286 / 298 / 310 cycles per round of 8 MFMAs with 1 / 2 / 3 / 4 reads); ds_write_b128 of
    // the four sibling waves between a read and its use add +30 cycles per round at 3 per wave (12 per round), +67 at 6 per wave
    // (24 per round) - v3 issues 24 per K-STEP, 6 per round: ~ +15; sibling LDS-DMA pieces (4-8 per round) add nothing.  So the probe
    // accounts for 1 024 + 4 x (42 + 15) = 1 250 of the traced 1 396-cycle MFMA phase; no single mechanism measured here explains the rest.
    // Measured: tower level 29.5 -> 28.2 us, Conf_Fusion's conv 113 -> 114, 64 x 64 tile 49.5 -> 46: not routed.
    static_assert(WM * WN == 4 || WM * WN == 8, "4 or 8 consumer wavefronts");
    constexpr int CT = Geo::CT;                   // consumer threads; the producers follow
    constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
    constexpr bool H16 = Geo::H16;                // split-fp16 arithmetic (above)
    static_assert(!H16 || BK == 64, "split-fp16 rows are 64 hi + 64 lo halves");
    // PF = 5: split-fp16 with the FILTER tile moved by LDS-DMA.  The pre-split filter rows are copied to LDS unchanged, and the
    // producers' ds_write_b128 of them were two thirds of the 24 KB a k-step pushes through the VGPR -> LDS store path (~79 B/clk
    // per CU: 310 of the traced 560-cycle store phase the consumers end up waiting for).  Four extra wavefronts (one per SIMD) do
    // nothing but issue global_load_lds_dwordx4 for the filter rows of k-tile t + 4 into a ring of FIVE filter stages (the
    // activation tile keeps its three register-staged stages and its producers, which now move only the 8 KB that need splitting),
    // wait with a counted s_waitcnt vmcnt until the pieces of tile t + 2 have landed, and join the k-step's barrier.  A stage is
    // the same padded row image as before (17 chunks of 16 bytes per row: linear chunk c = 17 row + chunk, the 17th a pad that
    // receives a dummy load), so the consumers' fragment addresses do not change; 1 KiB pieces are c = 64 piece + lane.
    // PF = 6: BOTH operands by LDS-DMA.  The input map arrives ALREADY split (usot_conv_desc.x_split: per pixel and 64-channel block the
    // 64 hi halves then the 64 lo halves of 8 x value - the 256 bytes of the fp32 block, written by the producing kernel's epilogue,
    // y_split), so an activation row of a k-tile is as ready-made as a filter row: the four DMA wavefronts fetch both tiles (a padding
    // tap fetches 16 zero bytes), five stages each, and the producer wavefronts with their loads, conversions and ds_writes are gone.
    constexpr bool XDMA = Geo::XDMA, WDMA = Geo::WDMA;
    constexpr int NDW = Geo::NDW;                 // DMA wavefronts (a piece costs its wave ~200 cycles of issue - traced: 26 pieces per k-tile over twelve waves)
    constexpr int NSW = Geo::NSW;                 // filter stages (six on the all-DMA tiles and those whose activation producers run four k-tiles deep)
    constexpr int LA = NSW - 1;                   // the DMA runs LA k-tiles ahead
    constexpr int LD = Geo::LD;                   // LDS rows padded by four floats (the conflict-free XOR-swizzled rows measured slower: LAB_NOTEBOOK A.3)
    constexpr int CPR = BK / 4;
    constexpr int NPT = 64 * NPW;                 // producer threads
    constexpr int RPP = NPT / CPR;
    constexpr int XI = (BM + RPP - 1) / RPP, WI = (BN + RPP - 1) / RPP;
    constexpr int NR = BK / 16;
    constexpr int STAGE = (BM + BN) * LD;
    // LDS: without the filter DMA three stages of [activation rows | filter rows]; with it three activation stages, then NSW filter stages
    constexpr int NSX = Geo::NSX;                              // activation stages
    constexpr int XSTRIDE = WDMA ? BM * LD : STAGE;            // floats between activation stages
    constexpr int WBASE = WDMA ? NSX * BM * LD : BM * LD;      // first filter stage
    constexpr int WSTRIDE = WDMA ? BN * LD : STAGE;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    const bool producer = threadIdx.x >= CT;
    const int tid = producer ? (int)threadIdx.x - CT : (int)threadIdx.x;
    constexpr int NPTL = Geo::NPT;                // producer threads actually launched (none when the activations come by DMA)
    // index prologue: every divisor is a constant of the problem, divided by with its host-made multiplier and shift (fastdiv.h)
    const int tiles = q.tiles;
    const int b = xcd_remap(bid0, q.total);
    const int z = fd_div(b, q.d_tiles), t0 = b - z * tiles;
    const int g = fd_div(z, q.d_ksplit), ks = z - g * q.ksplit;
    const int tn0 = fd_div(t0, q.d_MT);
    const int bn0 = tn0 * BN, bm0 = (t0 - tn0 * q.MT) * BM;
    const int KT = q.ktb;
    const int cch = q.cch;
    const int kt0 = fd_div(KT * ks, q.d_ksplit);              // (KT * ksplit < 2^31: the launcher checks)
    const int kt1 = fd_div(KT * (ks + 1), q.d_ksplit);
    const int nt = kt1 - kt0;
    // ML = the rows this launch computes: M, or with n_dyn the rows of the live images.  A workgroup whose tile lies past them leaves
    // here - before LDS, the split-K slabs, the tickets or the ovf word are touched (every k-slice of a tile takes the same decision, so
    // the tickets stay zero); a tile that straddles ML treats the rows past it as rows past M: not loaded (zeros), not stored
    const int ML = q.n_dyn ? min(max(dyn_n - q.n_first, 0), q.N) * q.P : q.M;
    if (bm0 >= ML) return;

    if constexpr (WDMA) {
        if ((int)threadIdx.x >= CT + NPTL) {
            // ---------------- DMA wavefronts: the filter tile (PF = 5, 6) and, with PF = 6, the activation tile too
            const int dt = (int)threadIdx.x - CT - NPTL;
            const int dwv = __builtin_amdgcn_readfirstlane(dt >> 6), lane = dt & 63;
            constexpr int NCH = BN * 17;                       // 16-byte chunks of a filter stage: 16 data + 1 pad per row
            constexpr int NPIECE = (NCH + 63) / 64;            // 1 KiB pieces (64 lanes x 16 bytes)
            constexpr int MAXP = (NPIECE + NDW - 1) / NDW;
            constexpr int NCHX = BM * 17;                      // the activation stage likewise (PF = 6)
            constexpr int NPX = XDMA ? (NCHX + 63) / 64 : 0;
            constexpr int MAXPX = XDMA ? (NPX + NDW - 1) / NDW : 1;
            const float *__restrict__ wg = q.w + (long)g * q.w_gs + (long)kt0 * BK;
            const float *src[MAXP];
            bool live[MAXP];
            int mine = 0;                                      // pieces this wave moves per k-tile (wave-uniform)
#pragma unroll
            for (int q = 0; q < MAXP; ++q) {
                const int piece = dwv + q * NDW, c = 64 * piece + lane;
                live[q] = piece < NPIECE && c < NCH;
                const int row = c / 17, ch = c - row * 17, co = bn0 + row;
                const bool ok = live[q] && ch < 16 && co < p.Cout;
                src[q] = wg + (ok ? (long)co * p.K + ch * 4 : 0L);      // pad chunks and rows past Cout fetch the bank's first bytes
                mine += piece < NPIECE ? 1 : 0;
            }
            // activation pieces: lane -> (pixel row of the tile, 16-byte chunk of its 64-channel block); the tap moves per k-tile
            const float *__restrict__ xg = p.x + (long)g * p.x_gs;
            int xih0[MAXPX], xiw0[MAXPX], xch[MAXPX];
            long xnb[MAXPX];
            bool xlive[MAXPX], xrow[MAXPX];
            if constexpr (XDMA) {
#pragma unroll
                for (int q = 0; q < MAXPX; ++q) {
                    const int piece = dwv + q * NDW, c = 64 * piece + lane;
                    xlive[q] = piece < NPX && c < NCHX;
                    const int row = c / 17, ch = c - row * 17, m = bm0 + row;
                    xrow[q] = xlive[q] && ch < 16 && m < ML;          // a real pixel and a data chunk (else: zeros)
                    const int mm = xrow[q] ? m : 0;
                    const int n = mm / p.P, pix = mm - n * p.P;
                    const int oh = pix / p.OW, ow = pix - oh * p.OW;
                    xih0[q] = oh * p.stride - p.pad_h;
                    xiw0[q] = ow * p.stride - p.pad_w;
                    xnb[q] = (long)n * p.H * p.W * p.Cin;
                    xch[q] = ch * 4;
                    mine += piece < NPX ? 1 : 0;
                }
            }
            const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void *)(smem + WBASE);
            const uint32_t ldsx = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void *)smem;
            auto dma = [&](const float *sp, uint32_t dst) {
                unsigned keep;
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(sp), "s"(dst) : "memory");
            };
            auto issue = [&](int tile) {                       // k-tile `tile` of this workgroup's range -> stage tile % NSW
                const uint32_t stg = lds0 + (uint32_t)((tile % NSW) * BN * LD * 4);
#pragma unroll
                for (int q = 0; q < MAXP; ++q) {
                    const int piece = dwv + q * NDW;
                    if (piece < NPIECE && live[q])
                        dma(src[q] + (long)tile * BK, __builtin_amdgcn_readfirstlane(stg + (uint32_t)(piece * 1024)));
                }
                if constexpr (XDMA) {
                    const int kt = kt0 + tile, tap = kt / cch, cc = kt - tap * cch;
                    const int kh = tap / p.KW, kw = tap - kh * p.KW;
                    const uint32_t stx = ldsx + (uint32_t)((tile % NSX) * BM * LD * 4);
#pragma unroll
                    for (int q = 0; q < MAXPX; ++q) {
                        const int piece = dwv + q * NDW;
                        if (piece < NPX && xlive[q]) {
                            const int ih = xih0[q] + kh * p.dil_h, iw = xiw0[q] + kw * p.dil_w;
                            const bool in = xrow[q] && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
                            const float *sp = in ? xg + xnb[q] + ((long)ih * p.W + iw) * p.Cin + cc * BK + xch[q] : p.zero;
                            dma(sp, __builtin_amdgcn_readfirstlane(stx + (uint32_t)(piece * 1024)));
                        }
                    }
                }
            };
            // at most the pieces of the LA - 2 newest k-tiles may stay in flight (drain = true: none - the tail, where fewer exist)
            auto land = [&](bool drain) {
                if (drain) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); return; }
                switch (mine) {
                case 1: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(1 * (LA - 2)) : "memory"); break;
                case 2: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * (LA - 2)) : "memory"); break;
                case 3: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(3 * (LA - 2)) : "memory"); break;
                case 4: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(4 * (LA - 2)) : "memory"); break;
                case 5: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(5 * (LA - 2)) : "memory"); break;
                case 6: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(6 * (LA - 2)) : "memory"); break;
                case 7: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(7 * (LA - 2)) : "memory"); break;
                case 8: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(8 * (LA - 2)) : "memory"); break;
                case 9: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(9 * (LA - 2)) : "memory"); break;
                case 10: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(10 * (LA - 2)) : "memory"); break;
                default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
                }
            };
            for (int j = 0; j < LA && j < nt; ++j) issue(j);
            land(nt < LA);                                     // k-tiles 0 and 1 are in LDS before the first barrier
            asm volatile("s_barrier" ::: "memory");
#ifdef USOT_TRACE
            unsigned *trd = (XDMA && p.ksplit == 1 && p.ws && bid0 == 0 && dt == 0) ? (unsigned *)p.ws : nullptr;
#define USOT_DSTAMP(slot, t) if (trd && (t) < 64) trd[(t) * 8 + (slot)] = (unsigned)__builtin_readcyclecounter()
#else
#define USOT_DSTAMP(slot, t)
#endif
            for (int t = 0; t < nt; ++t) {
                const bool more = t + LA < nt;
                USOT_DSTAMP(4, t);
                if (more) issue(t + LA);
                USOT_DSTAMP(3, t);
                USOT_DSTAMP(5, t);
                land(!more);                                   // k-tile t + 2 has landed when the consumers pass this step's barrier
                USOT_DSTAMP(6, t);
                asm volatile("s_barrier" ::: "memory");
                USOT_DSTAMP(7, t);
            }
#undef USOT_DSTAMP
            return;
        }
    }

    if (producer) {
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
            x_ok[i] = (row < BM) && (m < ML);
            const int mm = x_ok[i] ? m : 0;
            const int n = fd_div(mm, q.d_P), pix = mm - n * q.P;
            const int oh = fd_div(pix, q.d_OW), ow = pix - oh * q.OW;
            x_ih0[i] = oh * q.stride - q.pad_h;
            x_iw0[i] = ow * q.stride - q.pad_w;
            x_nb[i] = (long)n * q.H * q.W * q.Cin + kc * 4;
        }
        const float *wp[WI];
#pragma unroll
        for (int i = 0; i < WI; ++i) {
            const int row = lr + RPP * i;
            const int co = bn0 + row;
            wp[i] = wg + (long)((row < BN && co < q.Cout) ? co : 0) * q.K + kc * 4 + (long)kt0 * BK;
        }
        f32x4 xr[D][XI], wr[D][WI];
        bool xz[D][XI];
        const float *xp[XI];
        bool xin[XI];
        int cur_tap = fd_div(kt0, q.d_cch), cur_cc = kt0 - cur_tap * cch;
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
        auto load_tile = [&](auto dc, bool advance) {
            constexpr int d = decltype(dc)::value;
            const int c0 = cur_cc * BK;
#pragma unroll
            for (int i = 0; i < XI; ++i) {
                // unconditional load (padding taps read pixel 0 of the tensor and are zeroed at the
                // LDS store): a branch around the load makes the compiler's vmcnt bookkeeping
                // conservative and every buffer's last store then drains ALL loads in flight
#ifdef USOT_ABL_NOLOAD     // scripts/ablate_kstep.py: timing builds with parts of the kernel removed
                xr[d][i] = f32x4{1.f, 1.f, 1.f, 1.f};
#else
                xr[d][i] = *(const f32x4 *)(xin[i] ? xp[i] + c0 : xg + kc * 4);
#endif
                xz[d][i] = xin[i];
            }
            if constexpr (!WDMA) {
#pragma unroll
            for (int i = 0; i < WI; ++i) {
#if defined(USOT_ABL_NOLOAD) || defined(USOT_ABL_NOW) || defined(USOT_ABL_NOWLOAD)   // NOW: the W operand never travels; NOWLOAD / NOWSTORE / NOWREAD: one leg of it removed
                wr[d][i] = f32x4{1.f, 1.f, 1.f, 1.f};
#else
                wr[d][i] = *(const f32x4 *)wp[i];
#endif
                wp[i] += advance ? BK : 0;
            }
            }
            if (advance && ++cur_cc == cch) {
                cur_cc = 0;
                set_tap(++cur_tap);
            }
        };
        auto store_tile = [&](auto dc, int st) {
            constexpr int d = decltype(dc)::value;
            float *sX = smem + st * XSTRIDE, *sW = smem + WBASE + st * WSTRIDE;
#ifdef USOT_ABL_NOSTORE
            return;
#endif
            const int kcs = kc * 4;
#pragma unroll
            for (int i = 0; i < XI; ++i)
                if (BM % RPP == 0 || lr + RPP * i < BM) {
                    if constexpr (H16) {
                        // hi = fp16(8 x), lo = fp16(8 x - hi): halves kc*4 .. kc*4+3 of the row's hi plane and of its lo plane
                        const f32x4 v = (xz[d][i] ? xr[d][i] : f32x4{0.f, 0.f, 0.f, 0.f}) * 8.0f;
                        const uint32_t hi0 = usot_pack2_lp<true>(v[0], v[1]), hi1 = usot_pack2_lp<true>(v[2], v[3]);
                        const usot_f16x2 h0 = __builtin_bit_cast(usot_f16x2, hi0), h1 = __builtin_bit_cast(usot_f16x2, hi1);
                        const uint32_t lo0 = usot_pack2_lp<true>(v[0] - (float)h0[0], v[1] - (float)h0[1]);
                        const uint32_t lo1 = usot_pack2_lp<true>(v[2] - (float)h1[0], v[3] - (float)h1[1]);
                        const u32x2_t hi = {hi0, hi1}, lo = {lo0, lo1};
                        char *row = (char *)(sX + (lr + RPP * i) * LD);
                        *(u32x2_t *)(row + kc * 8) = hi;
                        *(u32x2_t *)(row + 128 + kc * 8) = lo;
                    } else {
                        *(f32x4 *)(sX + (lr + RPP * i) * LD + kcs) = xz[d][i] ? xr[d][i] : f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                }
#if !defined(USOT_ABL_NOW) && !defined(USOT_ABL_NOWSTORE)
            if constexpr (!WDMA) {
#pragma unroll
            for (int i = 0; i < WI; ++i)
                if (BN % RPP == 0 || lr + RPP * i < BN) *(f32x4 *)(sW + (lr + RPP * i) * LD + kcs) = wr[d][i];
            }
#elif defined(USOT_ABL_NOWSTORE)
#pragma unroll
            for (int i = 0; i < WI; ++i) {
                const f32x4 keep = wr[d][i];
                asm volatile("" :: "v"(keep));     // the loads stay, waited for here
            }
#endif
        };
        using I0 = std::integral_constant<int, 0>;
        using I1 = std::integral_constant<int, D >= 2 ? 1 : 0>;
        // Every load below is unconditional (past the last tile the pointers stop advancing and the
        // last tile is simply fetched again, never stored): the compiler can then count exactly
        // how many younger loads are in flight and waits with vmcnt(N > 0) instead of draining.
        // tiles 0 and 1 go to stages 0 and 1 before the first barrier; tiles 2 .. D+1 stay in
        // flight in register buffers 0 .. D-1 (tile t+2 lives in buffer t % D).  D up to 6: at batch 1 both
        // operands of a layer are cold (filters from the Infinity Cache / HBM once per frame, the activation
        // map from the other XCDs' write-backs), a round trip is 2-3 k-steps long.
        int lt = 0;                                   // next tile to fetch
        auto load_next = [&](auto dc) { load_tile(dc, lt + 1 < nt); ++lt; };
#ifdef USOT_TRACE
        unsigned tr_load = 0, tr_barrier = 0;
#define USOT_START(v) v = (unsigned)__builtin_readcyclecounter()
#else
#define USOT_START(v)
#endif
        if constexpr (D == 1) {
            load_next(I0{}); store_tile(I0{}, 0);
            USOT_START(tr_load);
            load_next(I0{}); if (nt > 1) store_tile(I0{}, 1);
        } else {
            load_next(I0{});
            load_next(I1{});
            USOT_START(tr_load);                      // the x and w loads of k-tiles 0 and 1 are issued
            store_tile(I0{}, 0);
            if (nt > 1) store_tile(I1{}, 1);
        }
        auto each_buffer = [&](auto f) {              // f(buffer index constant) for buffers 0 .. D-1, in order
            [&]<int... Is>(std::integer_sequence<int, Is...>) { (f(std::integral_constant<int, Is>{}), ...); }
            (std::make_integer_sequence<int, D>{});
        };
        each_buffer([&](auto dc) { load_next(dc); });
        __syncthreads();
        int st2 = 2;                                  // stage that receives tile t+2
#ifdef USOT_TRACE   // scripts/trace_kstep.py: s_memtime stamps of one producer wave into the (unused) split-K workspace
        USOT_START(tr_barrier);
        unsigned *trc = (p.ksplit == 1 && p.ws && bid0 == 0 && tid == 0) ? (unsigned *)p.ws : nullptr;
#define USOT_STAMP(slot, t) if (trc && (t) < 64) trc[(t) * 8 + (slot)] = (unsigned)__builtin_readcyclecounter()
        // start-up stamps, row 60 of the table (layer3's 3x3 has 36 k-tiles): kernel entry, first four loads issued, first barrier passed;
        // the first k-step begins at row 0's slot 4
        if (trc) { trc[60 * 8 + 0] = tr_entry; trc[60 * 8 + 1] = tr_load; trc[60 * 8 + 2] = tr_barrier; }
#else
#define USOT_STAMP(slot, t)
#endif
        auto step = [&](auto dc, int t) {
            USOT_STAMP(4, t);
#ifdef USOT_TRACE
            {   // the wait for the oldest register buffer's loads, apart from the conversion / store instructions behind it
                constexpr int d_ = decltype(dc)::value;
                asm volatile("" :: "v"(xr[d_][XI - 1]));
                USOT_STAMP(3, t);
            }
#endif
            if (t + 2 < nt) store_tile(dc, st2);
            USOT_STAMP(5, t);
            load_next(dc);
            USOT_STAMP(6, t);
            st2 = st2 == 2 ? 0 : st2 + 1;
#ifndef USOT_ABL_NOBARRIER      // timing only: producers and consumers free-running (results are garbage)
            __syncthreads();
#endif
            USOT_STAMP(7, t);
        };
        int t = 0;
        for (; t + D <= nt; t += D) each_buffer([&](auto dc) { step(dc, t + decltype(dc)::value); });
        each_buffer([&](auto dc) {                    // tail: t is a multiple of D here, buffers continue 0, 1, ...
            if (t < nt) { step(dc, t); ++t; }
        });
        return;
    }

    // ---------------- consumers
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const int l15 = lane & 15, quad = lane >> 4;
    const int fx_off = (wm * TM * 16 + l15) * LD + quad * 4;
    const int fw_off = BM * LD + (wn * TN * 16 + l15) * LD + quad * 4;
    constexpr int NSLOT = PF >= 2 ? NR : 2;
    static_assert(PF == 1 || (PF >= 2 && NR == 4), "PF >= 2 needs BK = 64");
    // split-fp16: the three products of one 32-k step on the blocks of this wave (slot ks = hi halves of k-step ks, slot ks + 2 = lo);
    // smallest terms first; a wave with a single block keeps the two cross terms on a second accumulator (no dependent chain of three)
    auto mma_h = [&](f32x4 (&a)[TN][TM], f32x4 &a2, const f32x4 (&whi)[TN], const f32x4 (&wlo)[TN], const f32x4 (&xhi)[TM], const f32x4 (&xlo)[TM], bool first) {
#ifdef USOT_ABL_NOMMA
        return;
#endif
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        auto h = [](const f32x4 &v) { return __builtin_bit_cast(f16x8_t, v); };
        if constexpr (TN * TM == 1) {
            a2      = __builtin_amdgcn_mfma_f32_16x16x32_f16(h(wlo[0]), h(xhi[0]), first ? zero : a2, 0, 0, 0);
            a[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(h(whi[0]), h(xhi[0]), first ? zero : a[0][0], 0, 0, 0);
            a2      = __builtin_amdgcn_mfma_f32_16x16x32_f16(h(whi[0]), h(xlo[0]), a2, 0, 0, 0);
        } else {
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j) a[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(h(wlo[i]), h(xhi[j]), first ? zero : a[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j) a[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(h(whi[i]), h(xlo[j]), a[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j) a[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(h(whi[i]), h(xhi[j]), a[i][j], 0, 0, 0);
        }
    };
    f32x4 fw[NSLOT][TN], fx[NSLOT][TM];
    auto read_frags = [&](int st, int r, int slot, int stw = 0) {       // stw: the filter stage (filter-DMA tiles only)
#ifdef USOT_ABL_NOREAD
        return;
#endif
        const float *base = smem + st * XSTRIDE + r * 16;
        const float *wbase = WDMA ? smem + WBASE - BM * LD + stw * WSTRIDE + r * 16 : base;     // (fw_off carries BM * LD)
#if defined(USOT_ABL_NOW) || defined(USOT_ABL_NOWREAD)
#pragma unroll
        for (int i = 0; i < TN; ++i) fw[slot][i] = f32x4{1.f + st, 2.f, 3.f + r, 4.f};
#else
#pragma unroll
        for (int i = 0; i < TN; ++i) fw[slot][i] = *(const f32x4 *)(wbase + fw_off + i * 16 * LD);
#endif
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
    // Blocked accumulation (see blocked_mma above): `acc` holds ONE k-tile's partial sums (its first MFMA takes C = 0),
    // `tot` the running total the finished k-tile is added to right after the barrier, when its MFMAs have long retired.
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
    auto mma = [&](int slot, bool first) {
#ifdef USOT_ABL_NOMMA
        return;
#endif
        blocked_mma<TN, TM>(acc, acc2, fw[slot], fx[slot], first);
    };
    // bias and residual of this lane's outputs are fetched NOW, while the producers bring the first k-tiles:
    // loaded in the epilogue they add a dependent L2/HBM round trip to the tail of every layer, when no
    // other work is left to hide it.  (vectorised NHWC stores without split-K only.)
    const bool pre = q.vec_store && q.ksplit == 1;
    f32x4 pb[TN], pr[TN][TM];
    f32x4 psc[H16 ? TN : 1];                      // split-fp16: this lane's four output-channel scales per block, fetched up front too
#pragma unroll
    for (int i = 0; i < TN; ++i) {
        const int co = bn0 + (wn * TN + i) * 16 + quad * 4;
        const bool cok = pre && co + 3 < q.Cout;
        pb[i] = (cok && q.bias) ? *(const f32x4 *)(q.bias + (long)g * q.b_gs + co) : f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (H16) {
#pragma unroll
            for (int e = 0; e < 4; ++e) psc[i][e] = co + e < q.Cout ? q.wscale[(long)g * q.b_gs + co + e] : 0.f;      // (the bias' group stride: rows of the bank per group)
        }
#pragma unroll
        for (int j = 0; j < TM; ++j) {
            const int m = bm0 + (wm * TM + j) * 16 + l15;
            pr[i][j] = (cok && q.res && m < ML)
                           ? *(const f32x4 *)(q.res + (long)g * q.r_gs + (long)m * q.res_cstride + q.res_coff + co)
                           : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    __syncthreads();
#ifdef USOT_TRACE
    unsigned *trc = (p.ksplit == 1 && p.ws && bid0 == 0 && tid == 0) ? (unsigned *)p.ws : nullptr;
#endif
    // PF = 3: the consumer's fragment traffic scheduled BY HAND.  hipcc's schedule of the plain loop (PF = 1) re-uses a fragment
    // register right behind the MFMA that read it and waits for that read at once (ds_read_b128 v[34:37] ... s_waitcnt lgkmcnt(1) ...
    // v_mfma ... v34), with s_nop 6-7 in front of reads that overwrite MFMA sources: the software pipeline of the source is gone
    // in the ISA.  Here the reads are inline asm (the compiler neither moves them behind their MFMAs nor waits for them), issued TWO
    // rounds ahead into one slot per round, and every round waits with a COUNTED s_waitcnt lgkmcnt(2 x reads per round) that carries
    // the round's fragment registers as operands, so no MFMA of the round can be scheduled above it.
    // (the registers travel as PARAMETERS: clang rejects asm operands that name captured arrays inside a generic lambda)
    auto aread_ = [](f32x4 (&w)[TN], f32x4 (&x)[TM], unsigned bw, unsigned bx, auto rc) {
        constexpr int r = decltype(rc)::value;
        constexpr int LD = BK + 4;                                // (a captureless lambda: the row length again)
#pragma unroll
        for (int i = 0; i < TN; ++i)
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(w[i]) : "v"(bw), "n"((i * 16 * LD + r * 16) * 4));
#pragma unroll
        for (int j = 0; j < TM; ++j)
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(x[j]) : "v"(bx), "n"((j * 16 * LD + r * 16) * 4));
    };
    auto aread = [&](int st, auto rc, auto sc) {
        aread_(fw[decltype(sc)::value], fx[decltype(sc)::value], (unsigned)((st * STAGE + fw_off) * 4), (unsigned)((st * STAGE + fx_off) * 4), rc);
    };
    auto await_ = [](f32x4 (&w)[TN], f32x4 (&x)[TM], auto nc) {   // wait until at most nc reads are outstanding; ties the slot's registers to the wait
        static_assert(TN <= 2 && TM <= 2, "operand list below");
        if constexpr (TN == 2 && TM == 1) asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(w[0]), "+v"(w[1]), "+v"(x[0]) : "n"(decltype(nc)::value));
        else if constexpr (TN == 1 && TM == 1) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(w[0]), "+v"(x[0]) : "n"(decltype(nc)::value));
        else if constexpr (TN == 1 && TM == 2) asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(w[0]), "+v"(x[0]), "+v"(x[1]) : "n"(decltype(nc)::value));
        else asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(w[0]), "+v"(w[1]), "+v"(x[0]), "+v"(x[1]) : "n"(decltype(nc)::value));
    };
    auto await_slot = [&](auto sc, auto nc) { await_(fw[decltype(sc)::value], fx[decltype(sc)::value], nc); };
    using R0 = std::integral_constant<int, 0>; using R1 = std::integral_constant<int, 1>;
    using R2 = std::integral_constant<int, 2>; using R3 = std::integral_constant<int, 3>;
    int stw = 0;                                  // filter stage of k-tile t (filter-DMA tiles: t % NSW)
    if constexpr (H16) {
        if (nt > 0) { read_frags(0, 0, 0); read_frags(0, 2, 2); read_frags(0, 1, 1); read_frags(0, 3, 3); }
    } else if constexpr (PF == 3) {
        if (nt > 0) { aread(0, R0{}, R0{}); aread(0, R1{}, R1{}); }
    } else {
        if (nt > 0) read_frags(0, 0, 0);
        if (PF == 2 && nt > 0) read_frags(0, 1, 1);
    }
    int st = 0;
    for (int t = 0; t < nt; ++t) {
        const int st1 = st == 2 ? 0 : st + 1;
        USOT_STAMP(0, t);
        flush();                                      // the previous k-tile's block (zeros at t = 0)
        if constexpr (H16) {
            // tile t + 1 is complete in its stage since the barrier that ended step t - 1 (the producers run two tiles ahead): its
            // fragments are fetched as soon as a slot pair is free
            const bool more = t + 1 < nt;
            const int stw1 = stw == NSW - 1 ? 0 : stw + 1;
            const int sx1 = XDMA ? stw1 : st1;            // (PF = 6: the activation ring is as deep as the filter ring)
            mma_h(acc, acc2, fw[0], fw[2], fx[0], fx[2], true);
            if (more) { read_frags(sx1, 0, 0, stw1); read_frags(sx1, 2, 2, stw1); }
            mma_h(acc, acc2, fw[1], fw[3], fx[1], fx[3], false);
            if (more) { read_frags(sx1, 1, 1, stw1); read_frags(sx1, 3, 3, stw1); }
            st = st1;
            stw = stw1;
            USOT_STAMP(1, t);
            __syncthreads();
            USOT_STAMP(2, t);
            continue;
        }
        if constexpr (PF == 3) {
            constexpr int RPR = TN + TM;              // reads per round
            using W2 = std::integral_constant<int, 2 * RPR>;
            const bool more = t + 1 < nt;
            aread(st, R2{}, R2{});  await_slot(R0{}, W2{}); mma(0, true);
            aread(st, R3{}, R3{});  await_slot(R1{}, W2{}); mma(1, false);
            if (more) {
                aread(st1, R0{}, R0{}); await_slot(R2{}, W2{}); mma(2, false);
                aread(st1, R1{}, R1{}); await_slot(R3{}, W2{}); mma(3, false);
            } else {                                   // last k-tile: nothing left to fetch, the two newest rounds drain
                await_slot(R2{}, std::integral_constant<int, RPR>{}); mma(2, false);
                await_slot(R3{}, R0{}); mma(3, false);
            }
            st = st1;
            USOT_STAMP(1, t);
            asm volatile("s_barrier" ::: "memory");   // not __syncthreads(): its lgkmcnt(0) would drain the reads in flight for tile t + 1
            USOT_STAMP(2, t);
            continue;
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            if constexpr (PF == 2) {
                // tile t + 1 is complete in its stage since the barrier that ended step t - 1 (the producers run two tiles ahead)
                if (r + 2 < NR) read_frags(st, r + 2, r + 2);
                else if (t + 1 < nt) read_frags(st1, r + 2 - NR, r + 2 - NR);
                __builtin_amdgcn_sched_barrier(0);
                mma(r, r == 0);
            } else {
                if (r + 1 < NR) read_frags(st, r + 1, (r + 1) & 1);
                else if (t + 1 < nt) read_frags(st1, 0, 0);
                mma(r & 1, r == 0);
            }
        }
        st = st1;
        USOT_STAMP(1, t);
#ifndef USOT_ABL_NOBARRIER
        __syncthreads();
#endif
        USOT_STAMP(2, t);
    }
#undef USOT_STAMP
#undef USOT_START
    flush();
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = tot[i][j].get();
    if constexpr (H16) {
        // back to the unscaled sums (powers of two: exact) before the split-K slabs, the deferred reduction or the epilogue see them
#pragma unroll
        for (int i = 0; i < TN; ++i)
#pragma unroll
            for (int j = 0; j < TM; ++j) acc[i][j] *= psc[i];
        // Range contract, enforced: an activation beyond the fp16 window was staged as hi = inf, lo = -inf and every sum it entered is
        // NaN (inf - inf) by now; the epilogues below would turn that into a FINITE number (fmaxf(NaN, 0) = 0, exp(0) = 1).  Say so in
        // the caller's sticky word before bias / activation / the split-K slabs see the sums: the engine re-runs the frame on the
        // exact-fp32 tiles.  One class test per accumulator register, once per launch - nothing in the k-loop.
        if (p.ovf) {
            bool bad = false;
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) bad |= !(__builtin_fabsf(acc[i][j][e]) <= 3.4028234664e38f);
            if (bad) __hip_atomic_store(p.ovf, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }

    if (p.ksplit > 1) {
#pragma unroll
        for (int j = 0; j < TM; ++j) {
            const int m = bm0 + (wm * TM + j) * 16 + l15;
            if (m >= ML) continue;
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
        if (p.combine) splitk_combine<BM, BN>(p, g, t0, tiles, bm0, bn0, tid, (int *)smem, ML);
        return;
    }
    const float *__restrict__ bg = p.bias ? p.bias + (long)g * p.b_gs : nullptr;
    const float *__restrict__ rg = p.res ? p.res + (long)g * p.r_gs : nullptr;
    float *__restrict__ yg = p.y + (long)g * p.y_gs;
#pragma unroll
    for (int j = 0; j < TM; ++j) {
        const int m = bm0 + (wm * TM + j) * 16 + l15;
        if (m >= ML) continue;
#pragma unroll
        for (int i = 0; i < TN; ++i) {
            const int co = bn0 + (wn * TN + i) * 16 + quad * 4;
            if (co >= p.Cout) continue;
            f32x4 v = acc[i][j];
            if (p.vec_store && co + 3 < p.Cout) {
                v += pb[i] + pr[i][j];                      // prefetched above (zeros where absent)
                const int a = co < p.act_split ? p.act : p.act2;
                if (a != USOT_ACT_NONE) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = apply_act(v[e], a);
                }
                if constexpr (H16) {
                    if (p.y_split) {
                        // the result leaves split (usot_conv_desc.y_split): per pixel and 64-channel block 64 hi halves then 64 lo halves of
                        // 8 x value - what a PF = 6 consumer's DMA copies into its LDS rows unchanged
                        const f32x4 w8 = v * 8.0f;
                        const uint32_t hi0 = usot_pack2_lp<true>(w8[0], w8[1]), hi1 = usot_pack2_lp<true>(w8[2], w8[3]);
                        const usot_f16x2 h0 = __builtin_bit_cast(usot_f16x2, hi0), h1 = __builtin_bit_cast(usot_f16x2, hi1);
                        const uint32_t lo0 = usot_pack2_lp<true>(w8[0] - (float)h0[0], w8[1] - (float)h0[1]);
                        const uint32_t lo1 = usot_pack2_lp<true>(w8[2] - (float)h1[0], w8[3] - (float)h1[1]);
                        char *blk = (char *)(yg + (long)m * p.y_cstride + p.y_coff + (co & ~63));
                        *(u32x2_t *)(blk + (co & 63) * 2) = u32x2_t{hi0, hi1};
                        *(u32x2_t *)(blk + 128 + (co & 63) * 2) = u32x2_t{lo0, lo1};
                        continue;
                    }
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
