// Convolution as implicit GEMM on the gfx950 fp32 matrix cores.
//
// GEMM view (per group):  D[co][m] = sum_k Wp[co][k] * A[m][k]
//   m = (n, oh, ow) output pixel,  k = (kh, kw, ci) with ci innermost (NHWC input),
//   A[m][k] = x[n][oh*s - ph + kh*dh][ow*s - pw + kw*dw][ci]   (0 outside the image).
// The weight tile is the MFMA "A" operand and the activation tile the "B" operand, so a
// lane's four accumulator registers are four CONSECUTIVE output channels of one pixel:
// the epilogue (bias, residual, activation) and the NHWC store are 16-byte accesses.
//
// v_mfma_f32_16x16x4_f32 is exact fp32 (an fmaf chain, one rounding per product) at
// 64 FLOP/clk/SIMD = 157.3 TFLOP/s chip peak: this is the roofline the fp32 path is
// measured against.  Each lane feeds it one float of W and one of A per instruction; a
// lane reads 4 consecutive k of its row with one ds_read_b128 and issues 4 MFMAs from
// it (lane quad q owns k-slot q of every 4x16 step, so a 16-wide k round costs one
// b128 read per 16x16 block row/column).
//
// Tiling: 256 threads = 4 wavefronts; workgroup tile BM(pixels) x BN(channels) x 32(k);
// register-staged double buffering: global loads for tile t+1 are issued before the
// MFMAs of tile t and written to the other LDS buffer after them; one barrier per tile.
// LDS rows are padded to 36 floats (144 B, keeps 16-B alignment, spreads rows over banks).
// Small M (batch 1: M = 961 or 625) is handled by small tiles and optional split-K, not
// by padding up to a big tile — see DESIGN.md "filling 1024 SIMDs at M = 961".
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <stdio.h>
#include <type_traits>
#include "usot_hip.h"
#include "common.h"

// This file holds the tile table and the host side (queries, pack_wfrag, fill_params, the launcher).  The kernels live in one header
// per generation: the routed ones beside this file, the families no tuning table routes under lab/ (experiments builds only).
#include "conv_f32_common.h"        // ConvK, ConvBatch, the epilogue / split-K / blocked_mma helpers

namespace {

// What a tile IS, in one row: family, name, launch shape (the family's geometry struct: what the kernel's launch bounds and LDS offsets
// read) and descriptor contract.  The launcher and the usot_conv_tile_* queries read these fields; nothing is inferred from combinations.
enum Family { F_NONE = 0, F_V1, F_V2, F_V3, F_V3P, F_WS, F_WSTAT };    // an empty slot; conv_igemm_f32, _v2, _v3, _v3p, _ws, conv_wstat_f32
struct SkInfo;                                      // lab/conv_f32_streamk.h
struct TileCfg {
    Family family; const char *name;                // name: what usot_conv_tile_name answers, the key of profiles/pmc_*.json
    int bm, bn, bk, ksw, threads, lds_bytes;
    int wfrag; bool xsplit;                         // the usot_conv_desc.w_frag the tile requires (0, 1, 2); reads usot_conv_desc.x_split
    int nst, rps;                                   // weight-stationary: serves K = nst * 128 * rps only
    void (*fn)(const ConvBatch); void (*skfn)(const ConvBatch, const SkInfo);      // skfn: the persistent stream-K family's kernel (fn is null)
    bool dyn() const { return family == F_V3; }     // honours usot_conv_desc.n_dyn
};
#define GEOM(...) __VA_ARGS__::threads, __VA_ARGS__::lds_bytes

}  // namespace

#include "conv_f32_v1.h"            // conv_igemm_f32
#include "conv_f32_v2.h"            // conv_igemm_f32_v2
#include "conv_f32_v3.h"            // conv_igemm_f32_v3 (exact fp32 and split-fp16)
#ifdef USOT_EXPERIMENTS             // each with its kTiles row macro and, where it has one, its launcher branch
#include "lab/conv_f32_streamk.h"   // conv_igemm_f32_v3p, tiles 72-78
#include "lab/conv_f32_wstream.h"   // conv_igemm_f32_ws, tiles 61-65
#include "lab/conv_f32_wstat.h"     // conv_wstat_f32, tiles 68-71
#endif

namespace {

#define TILE(bm, bn, wm, wn) { F_V1, "conv_igemm_f32<" #bm "," #bn ">", bm, bn, 32, 1, GEOM(V1Geom<bm, bn>), 0, false, 0, 0, conv_igemm_f32<bm, bn, wm, wn>, nullptr }
#define TILE2(bm, bn, wm, wn, bk) { F_V2, "conv_igemm_f32_v2<" #bm "," #bn ",BK=" #bk ">", bm, bn, bk, 1, GEOM(V2Geom<bm, bn, bk, 1>), 0, false, 0, 0, conv_igemm_f32_v2<bm, bn, wm, wn, bk>, nullptr }
#define TILE3(bm, bn, wm, wn, bk, ksw) { F_V2, "conv_igemm_f32_v2<" #bm "," #bn "," #bk "," #ksw "> ksw=" #ksw, bm, bn, bk, ksw, GEOM(V2Geom<bm, bn, bk, ksw>), 0, false, 0, 0, conv_igemm_f32_v2<bm, bn, wm, wn, bk, ksw>, nullptr }
#define V3ROW(tail, bm, bn, wm, wn, bk, d, npw, pf, wfrag) { F_V3, "conv_igemm_f32_v3<" #bm "," #bn ",BK=" #bk tail ">", bm, bn, bk, 1, GEOM(V3Geom<bm, bn, wm, wn, bk, d, npw, pf>), \
    wfrag, V3Geom<bm, bn, wm, wn, bk, d, npw, pf>::XDMA, 0, 0, conv_igemm_f32_v3<bm, bn, wm, wn, bk, d, npw, pf>, nullptr }
#define TILE4(bm, bn, wm, wn, bk) V3ROW("", bm, bn, wm, wn, bk, 1, 4, 1, 0)
#define TILE5(bm, bn, wm, wn, bk, d) V3ROW(",D=" #d, bm, bn, wm, wn, bk, d, 4, 1, 0)
#define TILE10(bm, bn, wm, wn, bk, d, npw) V3ROW(",D=" #d ",NPW=" #npw, bm, bn, wm, wn, bk, d, npw, 1, 0)
#define TILE11(bm, bn, wm, wn, bk, d, npw) V3ROW(",D=" #d ",NPW=" #npw ",PF=2", bm, bn, wm, wn, bk, d, npw, 2, 0)
#define TILE12(bm, bn, wm, wn, bk, d, npw) V3ROW(",D=" #d ",NPW=" #npw ",NCW=8", bm, bn, wm, wn, bk, d, npw, 1, 0)
#define TILE13(bm, bn, wm, wn, bk, d, npw) V3ROW(",D=" #d ",NPW=" #npw ",PF=3", bm, bn, wm, wn, bk, d, npw, 3, 0)
#define TILEH(bm, bn, wm, wn, d, npw) V3ROW(",D=" #d ",NPW=" #npw ",PF=4", bm, bn, wm, wn, 64, d, npw, 4, 2)
#define TILEHD(bm, bn, wm, wn, d, npw) V3ROW(",D=" #d ",NPW=" #npw ",PF=5", bm, bn, wm, wn, 64, d, npw, 5, 2)
#define TILEHX(bm, bn, wm, wn) V3ROW(",PF=6", bm, bn, wm, wn, 64, 2, 4, 6, 2)
// (TILEP, TILEW, TILES - the rows of the families without a routed tile - stand in their lab/ headers)
// One row per tile id (a new tile = a new row at the END: ids are positions; tests/test_conv_tile_table.py records every id's answers).
// The DEFAULT build compiles the ROUTED tiles only: the ids the tuning tables (usot_amd/data/tuning_gfx950.json, tuning_split16_gfx950.json),
// engine.SPLIT16_TILES, the engine's deferred-launch options and pick_tile() below can select.  The rule is pinned by
// tests/test_abi_and_build.py::test_default_library_holds_exactly_the_routed_conv_tiles, which asserts the two sets are equal.
// Every other id - the experiments the lab notebook records as "parity-green, measured slower, not routed" - keeps
// its NUMBER but is an empty slot unless the library is built with -DUSOT_EXPERIMENTS (usot_amd/build.py: USOT_EXPERIMENTS=1); the
// launcher answers USOT_ENOTBUILT for it and usot_conv_tile_built() says so up front.
#ifdef USOT_EXPERIMENTS
#define XT(...) __VA_ARGS__
#else
#define XT(...) TileCfg{}
#endif
const TileCfg kTiles[] = {
    TILE(128, 128, 2, 2),   // 1: batched backbone
    TILE(128, 64, 2, 2),    // 2
    XT(TILE(64, 128, 2, 2)),    // 3
    TILE(64, 64, 2, 2),     // 4
    TILE(32, 64, 2, 2),     // 5
    XT(TILE(64, 32, 2, 2)),     // 6
    TILE(32, 32, 2, 2),     // 7
    TILE(16, 64, 1, 4),     // 8: tiny M (template-side encoders)
    XT(TILE(16, 128, 1, 4)),    // 9
    XT(TILE(32, 128, 2, 2)),    // 10
    XT(TILE2(128, 128, 2, 2, 32)),  // 11: v2 (3-stage, mid-tile barrier)
    XT(TILE2(64, 64, 2, 2, 32)),    // 12
    XT(TILE2(64, 64, 2, 2, 64)),    // 13
    TILE2(32, 64, 2, 2, 32),    // 14
    TILE2(32, 64, 2, 2, 64),    // 15
    TILE2(32, 32, 2, 2, 64),    // 16
    XT(TILE2(64, 128, 2, 2, 32)),   // 17
    XT(TILE2(128, 64, 2, 2, 32)),   // 18
    XT(TILE2(32, 128, 2, 2, 32)),   // 19
    TILE2(16, 64, 1, 4, 64),    // 20
    XT(TILE2(64, 32, 2, 2, 64)),    // 21
    XT(TILE3(32, 64, 2, 2, 64, 2)), // 22: in-workgroup k-split, 8 waves
    XT(TILE3(32, 32, 2, 2, 64, 2)), // 23
    XT(TILE3(32, 32, 2, 2, 32, 4)), // 24: 16 waves
    XT(TILE3(64, 64, 2, 2, 32, 2)), // 25
    TILE3(16, 64, 1, 4, 64, 2), // 26
    XT(TILE3(32, 64, 2, 2, 32, 2)), // 27
    XT(TILE3(16, 64, 1, 4, 32, 4)), // 28
    TILE4(64, 64, 2, 2, 32),    // 29: v3 producer/consumer waves
    XT(TILE4(64, 64, 2, 2, 64)),    // 30
    TILE4(32, 64, 2, 2, 64),    // 31
    XT(TILE4(128, 128, 2, 2, 32)),  // 32
    TILE4(32, 32, 2, 2, 64),    // 33
    XT(TILE4(64, 128, 2, 2, 32)),   // 34
    XT(TILE4(128, 64, 2, 2, 32)),   // 35
    XT(TILE4(32, 128, 2, 2, 64)),   // 36
    XT(TILE5(64, 64, 2, 2, 32, 2)),    // 37: v3, two k-tiles of loads in flight per producer
    XT(TILE5(64, 64, 2, 2, 64, 2)),    // 38
    TILE5(32, 64, 2, 2, 64, 2),    // 39
    XT(TILE5(128, 128, 2, 2, 32, 2)),  // 40
    TILE5(32, 32, 2, 2, 64, 2),    // 41
    XT(TILE5(64, 128, 2, 2, 32, 2)),   // 42
    XT(TILE5(128, 64, 2, 2, 32, 2)),   // 43
    XT(TILE5(32, 128, 2, 2, 64, 2)),   // 44
    XT(TILE5(64, 64, 2, 2, 32, 3)),    // 45: three in flight
    XT(TILE5(64, 64, 2, 2, 64, 3)),    // 46
    XT(TILE5(32, 64, 2, 2, 64, 3)),    // 47
    XT(TILE5(128, 128, 2, 2, 32, 3)),  // 48
    TILE5(32, 32, 2, 2, 64, 3),    // 49
    XT(TILE5(64, 128, 2, 2, 32, 3)),   // 50
    XT(TILE5(128, 64, 2, 2, 32, 3)),   // 51
    XT(TILE5(32, 128, 2, 2, 64, 3)),   // 52
    TILE10(32, 32, 2, 2, 64, 2, 8),   // 53: eight producer waves
    TILE10(32, 32, 2, 2, 64, 3, 8),   // 54
    TILE10(32, 64, 2, 2, 64, 2, 8),   // 55
    TILE10(32, 64, 2, 2, 64, 3, 8),   // 56
    TILE10(64, 64, 2, 2, 64, 2, 8),   // 57
    XT(TILE10(64, 64, 2, 2, 32, 2, 8)),   // 58
    XT(TILE10(32, 128, 2, 2, 64, 2, 8)),  // 59
    XT(TILE10(64, 32, 2, 2, 64, 2, 8)),   // 60
    XT(TILEW(32, 64, 2, 4, 3, 1)),         // 61: weight-streaming consumers (filters in fragment order, usot_conv_pack_wfrag_f32); 1 x 4 waves
    XT(TILEW(32, 64, 2, 4, 2, 1)),         // 62
    XT(TILEW(64, 64, 2, 4, 3, 1)),         // 63
    XT(TILEW(32, 64, 2, 4, 2, 2)),         // 64: the same, consumer waves 2 x 2 (a wave pair shares its filter fragments through L1)
    XT(TILEW(64, 64, 2, 4, 2, 2)),         // 65
    XT(TILE11(32, 64, 2, 2, 64, 2, 4)),   // 66: v3 with fragment reads two rounds ahead (PF = 2)
    XT(TILE11(32, 32, 2, 2, 64, 2, 8)),   // 67
    XT(TILES(18, 1, false)),             // 68: weight-stationary, K = 2304 (3 x 3 x 256)
    XT(TILES(9, 1, false)),              // 69: K = 1152 (3 x 3 x 128)
    XT(TILES(18, 1, true)),             // 70: K = 2304, blocked accumulation (64-product blocks + running total)
    XT(TILES(8, 1, false)),              // 71: K = 1024
    XT(TILEP(64, 64, 2, 2, 2, 8, 64)),    // 72: v3 as a persistent stream-K launch (whole-chip rounds)
    XT(TILEP(32, 64, 2, 2, 2, 8, 64)),    // 73
    XT(TILEP(64, 64, 2, 2, 3, 8, 64)),    // 74
    XT(TILEP(64, 64, 2, 2, 2, 4, 64)),    // 75
    XT(TILEP(32, 32, 2, 2, 3, 8, 64)),    // 76
    XT(TILEP(64, 64, 2, 2, 2, 8, 32)),    // 77: k-tiles of 32
    XT(TILEP(128, 64, 2, 2, 2, 4, 32)),   // 78
    // (72-78, round 5: parity-green; Conf_Fusion's conv isolated 120 (v3 32 x 64) -> 111 us on tile 74 - 64 x 64 tiles without the
    //  three-round quantisation - but INSIDE the frame 111.6 -> 119.5 us and the graph +13 us; the three search encoders 74.6 -> 71.1
    //  per op, graph +10; shortcut conv + conv1 97 -> 132.  128 x 64 / 64 x 128 / 128 x 128 shapes spill at 768 threads.  Not in
    //  the tuning table)
    // (61-67: parity-green, none faster than v3 - DESIGN.md section 3.1 "what a k-step waits for")
    XT(TILE12(32, 64, 2, 4, 64, 2, 8)),   // 79: v3 with EIGHT consumer waves (two per SIMD) on the same tile: 16 x 16 wave tiles
    XT(TILE12(32, 64, 2, 4, 64, 3, 8)),   // 80
    XT(TILE12(64, 64, 2, 4, 64, 2, 8)),   // 81: 32 x 16 wave tiles
    XT(TILE12(64, 64, 4, 2, 64, 2, 8)),   // 82: 16 x 32
    XT(TILE12(64, 32, 4, 2, 64, 2, 8)),   // 83: 16 x 16
    XT(TILE12(32, 64, 2, 4, 64, 2, 4)),   // 84
    XT(TILE12(64, 64, 2, 4, 64, 3, 8)),   // 85
    XT(TILE13(32, 64, 2, 2, 64, 2, 8)),   // 86: v3 with the consumer's fragment reads hand-scheduled (PF = 3: asm reads two rounds ahead, counted waits)
    XT(TILE13(32, 64, 2, 2, 64, 3, 8)),   // 87
    XT(TILE13(32, 32, 2, 2, 64, 2, 8)),   // 88
    XT(TILE13(32, 32, 2, 2, 64, 3, 8)),   // 89
    XT(TILE13(64, 64, 2, 2, 64, 2, 8)),   // 90
    TILEH(32, 64, 2, 2, 2, 8),        // 91: v3 on SPLIT-fp16 arithmetic (PF = 4: filters pre-split, usot_conv_desc.w_frag = 2 + w_scale)
    TILEH(32, 64, 2, 2, 3, 8),        // 92
    XT(TILEH(32, 64, 2, 2, 4, 8)),        // 93
    TILEH(32, 32, 2, 2, 2, 8),        // 94
    TILEH(32, 32, 2, 2, 3, 8),        // 95
    XT(TILEH(32, 32, 2, 2, 4, 8)),        // 96
    TILEH(64, 64, 2, 2, 2, 8),        // 97
    XT(TILEH(64, 64, 2, 2, 3, 8)),        // 98
    TILEH(32, 64, 2, 2, 2, 4),        // 99
    XT(TILEH(32, 64, 2, 2, 4, 4)),        // 100
    XT(TILEH(64, 64, 2, 2, 4, 8)),        // 101
    XT(TILEH(32, 128, 2, 2, 2, 8)),       // 102
    XT(TILEH(64, 128, 2, 2, 2, 8)),       // 103
    TILEH(32, 32, 2, 2, 2, 4),        // 104
    XT(TILEHD(32, 64, 2, 2, 2, 4)),       // 105: split-fp16 with the filter tile moved by four LDS-DMA wavefronts into five stages (PF = 5)
    TILEHD(32, 64, 2, 2, 3, 4),       // 106
    TILEHD(32, 64, 2, 2, 2, 8),       // 107
    XT(TILEHD(32, 32, 2, 2, 2, 4)),       // 108
    XT(TILEHD(64, 64, 2, 2, 2, 4)),       // 109
    XT(TILEHD(64, 64, 2, 2, 2, 8)),       // 110
    TILEHD(32, 32, 2, 2, 3, 4),       // 111
    XT(TILEHD(64, 64, 2, 2, 3, 4)),       // 112
    XT(TILEHD(32, 64, 2, 2, 4, 4)),       // 113: D = 4 and SIX filter stages (the DMA five k-tiles ahead)
    XT(TILEHD(32, 32, 2, 2, 4, 4)),       // 114
    XT(TILEHD(32, 64, 2, 2, 4, 8)),       // 115
    XT(TILEHX(32, 64, 2, 2)),             // 116: split-fp16, BOTH operands by LDS-DMA (PF = 6): the input map arrives split (usot_conv_desc.x_split), no producer waves
    XT(TILEHX(32, 32, 2, 2)),             // 117
};
constexpr int kNumTiles = sizeof(kTiles) / sizeof(kTiles[0]);
const TileCfg &tile_row(int tile) { static const TileCfg none{}; return tile >= 1 && tile <= kNumTiles ? kTiles[tile - 1] : none; }      // out of range: an empty slot

int pick_tile(const usot_conv_desc *d, int M)
{
    // Aim for >= ~1 wave of workgroups (256 CUs, up to 4 resident per CU for the small
    // tiles) without shrinking below what the problem needs.
    const int order[] = {1, 2, 4, 5, 7};
    int best = 7;
    for (int id : order) {
        const TileCfg &t = kTiles[id - 1];
        if (t.bn > ((d->Cout + 15) / 16) * 16 && t.bn > 32) continue;
        long blocks = (long)((M + t.bm - 1) / t.bm) * ((d->Cout + t.bn - 1) / t.bn) * d->groups;
        if (blocks >= 512) { best = id; break; }
    }
    if (M <= 16 * 12) best = 8;
    return best;
}

}  // namespace

extern "C" int usot_conv_tile_count(void) { return kNumTiles; }

extern "C" int usot_conv_tile_built(int tile) { return tile_row(tile).family != F_NONE; }

extern "C" int usot_experiments_built(void)
{
#ifdef USOT_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}

extern "C" int usot_conv_tile_info(int tile, int *bm, int *bn)
{
    if (tile < 1 || tile > kNumTiles) return USOT_EINVAL;
    if (bm) *bm = kTiles[tile - 1].bm;
    if (bn) *bn = kTiles[tile - 1].bn;
    return USOT_OK;
}

/* kernel symbol of a tile id as rocprofv3 prints it (for matching bench.py's roofline object
 * with profiles/) */
extern "C" int usot_conv_tile_name(int tile, char *buf, int len)
{
    if (tile < 1 || tile > kNumTiles || !buf || len < 8) return USOT_EINVAL;
    const TileCfg &t = kTiles[tile - 1];
    if (t.name) snprintf(buf, len, "%s", t.name);
    else        snprintf(buf, len, "(tile %d: experiments build only)", tile);
    return USOT_OK;
}

/* workgroup size and dynamic LDS bytes of the tile's launch (zeros: not built): lets the table be checked without a GPU */
extern "C" int usot_conv_tile_launch(int tile, int *threads, int *lds_bytes)
{
    if (tile < 1 || tile > kNumTiles) return USOT_EINVAL;
    if (threads) *threads = kTiles[tile - 1].threads;
    if (lds_bytes) *lds_bytes = kTiles[tile - 1].lds_bytes;
    return USOT_OK;
}

/* 1 when the tile takes its filters in MFMA fragment order (usot_conv_pack_wfrag_f32, descriptor field w_frag = 1) */
extern "C" int usot_conv_tile_wfrag(int tile) { return tile_row(tile).wfrag; }

/* 1 when the tile honours usot_conv_desc.n_dyn: the producer / consumer family (conv_igemm_f32_v3), exact-fp32 and split-fp16 */
extern "C" int usot_conv_tile_dyn(int tile) { return tile_row(tile).dyn(); }
extern "C" int usot_conv_tile_xsplit(int tile) { return tile_row(tile).xsplit; }

/* weight-stationary tiles serve ONE reduction length: K the tile requires (0: any K the other rules allow); their other
 * requirements: Cin % kpanel == 0 (128 or 256, returned through *kpanel), Cout % 32 == 0, ksplit == 1, w_frag == 1 */
extern "C" int usot_conv_tile_kreq(int tile, int *kpanel)
{
    const TileCfg &t = tile_row(tile);
    if (kpanel && t.nst) *kpanel = 128 * t.rps;
    return t.nst * 128 * t.rps;
}

namespace {
__global__ void pack_wfrag_kernel(const float *__restrict__ w, float *__restrict__ wf, int Cout, int K, long n4)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;        // one float4 of the packed bank
    if (i >= n4) return;
    const int lane = (int)(i & 63);
    const long rest = i >> 6;
    const int r = (int)(rest & 3);
    const long tb = rest >> 2;                                          // cb * KT + kt
    const int KT = K / 64;
    const int kt = (int)(tb % KT), cb = (int)(tb / KT);
    const int row = cb * 16 + (lane & 15), col = kt * 64 + r * 16 + (lane >> 4) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row < Cout) v = *(const f32x4 *)(w + (long)row * K + col);
    *(f32x4 *)(wf + i * 4) = v;
}
}  // namespace

/* w [Cout][K] row-major (k = (kh*KW + kw)*Cin + ci, Cin % 64 == 0) -> wf: ceil(Cout/16) blocks of 16 x K floats in the order
 * [block][k-tile of 64][round of 16 k][lane = (k-slot quad)*16 + row][4 consecutive k]: what lane `lane` of a consumer
 * wave feeds v_mfma_f32_16x16x4_f32 as the A operand, one contiguous KiB per wave and round.  Rows past Cout are zero. */
extern "C" int usot_conv_pack_wfrag_f32(void *stream, const float *w, float *wf, int Cout, int K)
{
    if (!w || !wf || Cout < 1 || K < 64 || (K & 63)) return USOT_EINVAL;
    if (((uintptr_t)w | (uintptr_t)wf) & 15) return USOT_EINVAL;
    const long n4 = (long)((Cout + 15) / 16) * 16 * K / 4;
    hipLaunchKernelGGL(pack_wfrag_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, wf, Cout, K, n4);
    if (hipGetLastError() != hipSuccess) return USOT_ELAUNCH;
    return USOT_OK;
}

extern "C" int usot_conv_resolve_tile(const usot_conv_desc *d)
{
    if (!d) return USOT_EINVAL;
    if (d->tile != 0) return d->tile;
    return pick_tile(d, d->N * d->OH * d->OW);
}

extern "C" int64_t usot_conv_ws_floats(const usot_conv_desc *d)
{
    if (!d || d->ksplit <= 1) return 0;
    /* slabs + one ticket word per (group, tile) of the smallest tile shape (16 x 32) */
    const int64_t m = (int64_t)d->N * d->OH * d->OW;
    return (int64_t)d->ksplit * d->groups * m * d->Cout + (int64_t)d->groups * ((m + 15) / 16) * ((d->Cout + 31) / 32);
}

namespace {

// validates one descriptor and fills the kernel-side parameter block (tile-independent part)
int fill_params(const usot_conv_desc *d, ConvK &p)
{
    if (!d || !d->x || !d->w || !d->y) return USOT_EINVAL;
    if (d->Cin <= 0 || (d->Cin & 31) || d->Cout <= 0 || d->N <= 0) return USOT_EINVAL;
    if (d->groups < 1 || d->stride < 1 || d->KH < 1 || d->KW < 1) return USOT_EINVAL;
    const int oh = (d->H + 2 * d->pad_h - d->dil_h * (d->KH - 1) - 1) / d->stride + 1;
    const int ow = (d->W + 2 * d->pad_w - d->dil_w * (d->KW - 1) - 1) / d->stride + 1;
    if (oh != d->OH || ow != d->OW || oh <= 0 || ow <= 0) return USOT_EINVAL;
    const int ksplit = d->ksplit > 1 ? d->ksplit : 1;
    if (ksplit > 1 && !d->ws) return USOT_EINVAL;
    // the split-K slabs are addressed through a raw buffer descriptor with 32-bit byte offsets (ws_rsrc): past 2 GiB the
    // offsets would wrap and the accesses fall out of range silently
    if (ksplit > 1 && (int64_t)ksplit * (d->groups > 1 ? d->groups : 1) * d->N * oh * ow * d->Cout * 4 >= 0x7fffffffLL) return USOT_EINVAL;
    p.x = d->x; p.w = d->w; p.bias = d->bias; p.res = d->res; p.y = d->y; p.ws = d->ws;
    p.N = d->N; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.OH = d->OH; p.OW = d->OW; p.Cout = d->Cout;
    p.KH = d->KH; p.KW = d->KW; p.stride = d->stride; p.pad_h = d->pad_h; p.pad_w = d->pad_w;
    p.dil_h = d->dil_h; p.dil_w = d->dil_w;
    p.y_nchw = d->y_nchw;
    p.y_cstride = d->y_cstride > 0 ? d->y_cstride : d->Cout;
    p.y_coff = d->y_coff;
    p.res_cstride = d->res_cstride > 0 ? d->res_cstride : d->Cout;
    p.res_coff = d->res_coff;
    p.act = d->act; p.act2 = d->act2;
    p.act_split = d->act_split > 0 ? d->act_split : (1 << 30);
    p.groups = d->groups;
    p.x_gs = d->x_gs; p.w_gs = d->w_gs; p.b_gs = d->b_gs; p.y_gs = d->y_gs; p.r_gs = d->r_gs;
    p.ksplit = ksplit;
    if (d->defer && ksplit < 2) return USOT_EINVAL;
    p.combine = d->defer ? 0 : 1;            // deferred reduction: the slabs ARE the result (plain stores, no tickets)
    // rows, taps and reduction length are dividends of the kernels' multiply-and-shift divisions (fastdiv.h): exact below 2^31 only
    if ((int64_t)d->N * d->OH * d->OW > (int64_t)FASTDIV_MAX_DIVIDEND || (int64_t)d->KH * d->KW * d->Cin > (int64_t)FASTDIV_MAX_DIVIDEND)
        return USOT_EINVAL;
    p.P = d->OH * d->OW;
    p.M = d->N * p.P;
    p.K = d->KH * d->KW * d->Cin;
    p.cchunks = d->Cin / 32;
    p.KT = d->KH * d->KW * p.cchunks;
    p.wscale = nullptr; p.zero = nullptr; p.x_split = p.y_split = 0; p.ovf = nullptr;
    if (d->n_dyn && (((uintptr_t)d->n_dyn & 3) || d->n_first < 0)) return USOT_EINVAL;
    p.n_dyn = (const int *)d->n_dyn; p.n_first = d->n_first;
    p.vec_store = !d->y_nchw && (p.y_cstride % 4 == 0) && (p.y_coff % 4 == 0) &&
                  (!d->res || (p.res_cstride % 4 == 0 && p.res_coff % 4 == 0)) &&
                  ((uintptr_t)d->y % 16 == 0) && (!d->res || (uintptr_t)d->res % 16 == 0) &&
                  (!d->bias || (uintptr_t)d->bias % 16 == 0) &&
                  (d->y_gs % 4 == 0) && (d->r_gs % 4 == 0) && (d->b_gs % 4 == 0) &&
                  // the vector epilogues pick the activation once per group of four channels, from the group's first one: a split
                  // inside a group takes the per-channel scalar epilogue (the frame's act_split = 256 keeps the vector path)
                  (d->act_split <= 0 || d->act_split % 4 == 0 || d->act == d->act2);
    if (((uintptr_t)d->x % 16) || ((uintptr_t)d->w % 16) || (d->x_gs % 4) || (d->w_gs % 4))
        return USOT_EINVAL;
    return USOT_OK;
}

}  // namespace

/* workspace floats a persistent stream-K tile (usot_conv_tile_streamk(tile) == 1) needs for this batch of problems: the partial
 * tiles of the workgroup shares that end inside a tile + four ticket words per tile.  d[0].ws must hold that many floats, ZERO
 * before the first launch (the kernel leaves the tickets zero); 0 for the other tiles, negative = invalid arguments. */
extern "C" int64_t usot_conv_streamk_ws_floats(const usot_conv_desc *d, int n, int tile)
{
    if (!d || n < 1 || n > 4 || tile < 1 || tile > kNumTiles) return USOT_EINVAL;
    const TileCfg &tc = kTiles[tile - 1];
    if (tc.family != F_V3P) return 0;              // every tile of the default build
#ifdef USOT_EXPERIMENTS
    const int usot_dv = usot_device_slot();        // per-device launcher state (common.h)
    if (usot_dv < 0) return USOT_ESTATE;
    ConvBatch bt;
    SkInfo sk;
    bt.n = n;
    for (int i = 0; i < n; ++i) {
        usot_conv_desc c = d[i];
        if (!c.y) c.y = (float *)c.x;                  // sizing only
        int rc = fill_params(&c, bt.p[i]);
        if (rc != USOT_OK) return rc;
    }
    return sk_plan(tc, tile, d, n, bt, sk);
#else
    return 0;
#endif
}

extern "C" int usot_conv_tile_streamk(int tile) { return tile_row(tile).family == F_V3P; }

extern "C" int usot_conv2d_batch_f32(void *stream, const usot_conv_desc *d, int n)
{
    const int usot_dv = usot_device_slot();        // per-device launcher state below (common.h)
    if (usot_dv < 0) return USOT_ESTATE;
    if (!d || n < 1 || n > 4) return USOT_EINVAL;
    ConvBatch bt;
    bt.n = n;
    int rc;
    for (int i = 0; i < n; ++i)
        if ((rc = fill_params(&d[i], bt.p[i])) != USOT_OK) return rc;
    int tile = d[0].tile;
    if (tile == 0) {                       // heuristic on the largest problem
        int big = 0;
        for (int i = 1; i < n; ++i)
            if ((long)bt.p[i].M * bt.p[i].Cout * bt.p[i].K > (long)bt.p[big].M * bt.p[big].Cout * bt.p[big].K) big = i;
        tile = pick_tile(&d[big], bt.p[big].M);
    }
    if (tile < 1 || tile > kNumTiles) return USOT_EINVAL;
    const TileCfg &tc = kTiles[tile - 1];
    if (tc.family == F_NONE) return USOT_ENOTBUILT;
    long blocks = 0;
    // run-time image counts (usot_conv_desc.n_dyn): the producer / consumer tiles (conv_igemm_f32_v3, exact and split-fp16) only
    for (int i = 0; i < n; ++i)
        if (d[i].n_dyn && (!tc.dyn() || d[i].defer)) return USOT_EINVAL;
#ifdef USOT_EXPERIMENTS                    // the families with a launch of their own; without the define no row has either family
    if (tc.family == F_V3P) return launch_streamk(tc, tile, stream, d, n, bt);
    if (tc.family == F_WSTAT) return launch_wstat(tc, tile, stream, d, n, bt, usot_dv);
#endif
    for (int i = 0; i < n; ++i) {
        ConvK &p = bt.p[i];
        if (d[i].Cin % tc.bk) return USOT_EINVAL;
        if (p.ksplit > p.K / tc.bk) return USOT_EINVAL;
        // filters in fragment order iff the tile streams them (a row-major bank under a streaming tile, or the reverse,
        // would compute garbage silently); group strides must keep whole 16-row blocks
        if (d[i].w_frag != tc.wfrag) return USOT_EINVAL;
        if (tc.wfrag == 2 && (!d[i].w_scale || ((uintptr_t)d[i].w_scale & 3))) return USOT_EINVAL;
        p.wscale = d[i].w_scale;
        if ((uintptr_t)d[i].ovf & 3) return USOT_EINVAL;
        p.ovf = tc.wfrag == 2 ? d[i].ovf : nullptr;
        // split maps: only the split-fp16 tiles write them (vectorised NHWC epilogue, whole 64-channel blocks, no split-K), only the
        // all-DMA tiles read them - and those read nothing else
        p.x_split = d[i].x_split ? 1 : 0;
        p.y_split = d[i].y_split ? 1 : 0;
        if (p.x_split != (tc.xsplit ? 1 : 0)) return USOT_EINVAL;
        if (p.y_split && (tc.wfrag != 2 || !p.vec_store || (d[i].Cout & 63) || (p.y_coff & 63) || (p.y_cstride & 63) || p.ksplit > 1 || d[i].res)) return USOT_EINVAL;
        if (p.x_split) {
            static const float *zero_page_d[USOT_MAX_DEV] = {};
    const float *&zero_page = zero_page_d[usot_dv];
            if (!zero_page) {
                void *zp = nullptr;
                if (hipGetSymbolAddress(&zp, HIP_SYMBOL(g_zero16_f32)) != hipSuccess || !zp) return USOT_ELAUNCH;
                zero_page = (const float *)zp;
            }
            p.zero = zero_page;
        }
        if (tc.wfrag == 1 && p.groups > 1 && (p.w_gs % ((long)16 * p.K))) return USOT_EINVAL;
        p.MT = (p.M + tc.bm - 1) / tc.bm;
        p.NT = (d[i].Cout + tc.bn - 1) / tc.bn;
        // the rest of the prologue block (conv_f32_common.h: ConvPro): the tile's k-tile counts, the workgroup counts and the division
        // constants of every divisor the index prologue and the tap walk divide by.  Dividends: workgroup index < total, tile index
        // < tiles, row < M, pixel < P, k-tile bound <= ktb * ksplit, k-tile < ktb, tap < KH * KW - all kept below 2^31 here.
        const int64_t total = (int64_t)p.MT * p.NT * p.groups * p.ksplit;
        p.ktb = p.K / tc.bk;
        p.cch = d[i].Cin / tc.bk;
        if (total > (int64_t)FASTDIV_MAX_DIVIDEND || (int64_t)p.ktb * p.ksplit > (int64_t)FASTDIV_MAX_DIVIDEND) return USOT_EINVAL;
        p.tiles = p.MT * p.NT;
        p.total = (int)total;
        p.d_tiles = fastdiv_make((uint32_t)p.tiles);
        p.d_ksplit = fastdiv_make((uint32_t)p.ksplit);
        p.d_MT = fastdiv_make((uint32_t)p.MT);
        p.d_P = fastdiv_make((uint32_t)p.P);
        p.d_OW = fastdiv_make((uint32_t)p.OW);
        p.d_KW = fastdiv_make((uint32_t)p.KW);
        p.d_cch = fastdiv_make((uint32_t)p.cch);
        bt.start[i] = (int)blocks;
        blocks += total;
    }
    for (int i = n; i < 5; ++i) bt.start[i] = (int)blocks;
    if (blocks <= 0 || blocks > 0x7fffffffL) return USOT_EINVAL;
    if (tc.lds_bytes > 64 * 1024) {
        static bool raised_d[USOT_MAX_DEV][128] = {};
    bool (&raised)[128] = raised_d[usot_dv];
        if (!raised[tile]) {
            if (hipFuncSetAttribute((const void *)tc.fn, hipFuncAttributeMaxDynamicSharedMemorySize, tc.lds_bytes) != hipSuccess)
                return USOT_ELAUNCH;
            raised[tile] = true;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tc.fn, dim3((unsigned)blocks), dim3(tc.threads), tc.lds_bytes, s, bt);
    if (hipGetLastError() != hipSuccess) return USOT_ELAUNCH;
    return USOT_OK;
}

extern "C" int usot_conv2d_f32(void *stream, const usot_conv_desc *d)
{
    return usot_conv2d_batch_f32(stream, d, 1);
}
