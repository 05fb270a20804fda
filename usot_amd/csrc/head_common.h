// Device helpers shared by the single-frame head kernels (head_ops.hip) and their lock-step batched forms (multitrack.hip):
// one copy of the decode's argmax rule and of the SiamFC crop arithmetic, so that a batched slot is bit-identical to the
// single-frame kernel run on that slot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace usot_head {

// ---- decode (usot_tracker.py:138-163): the state one thread keeps for its best response cell
struct DecCell {
    double ps, x1, y1, x2, y2, pen;
    float sc;
    int i;
};

// np.argmax semantics (usot_tracker.py:163): first maximum, and a NaN counts as the maximum (the first NaN wins);
// index 0x7fffffff = "no cell" loses to everything
__device__ __forceinline__ bool dec_better(double ov, int oi, double mv, int mi)
{
    const bool on = ov != ov, mn = mv != mv;
    return oi != 0x7fffffff &&
        (mi == 0x7fffffff || (on && !mn) || (on == mn && (on ? oi < mi : (ov > mv || (ov == mv && oi < mi)))));
}

// ---- SiamFC crop on the device (lib/utils/track_utils.py:30-119): window extraction with
// mean-colour padding, OpenCV-style fixed-point bilinear resize (the arithmetic restated in
// usot_amd/hostutils.py::resize_bilinear_u8) and HWC uint8 -> CHW float32, one output pixel per call.
struct CropK {
    const unsigned char *im;      // [H][W][3]
    float *out;                   // [3][S][S]
    int H, W, S, win;
    int x0, y0;                   // window origin in image coordinates (may be negative)
    int fill[3];
};

__device__ __forceinline__ void crop_axis(int d, int n_src, int n_dst, int &s0, int &s1, int &w0, int &w1)
{
    // OpenCV's own arithmetic (see hostutils._resize_axis): double scale = 1 / (dst / src), the source
    // coordinate rounded to float BEFORE the floor, float fraction, round-half-even coefficients
    const double scale = 1.0 / ((double)n_dst / (double)n_src);
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.0f; s = 0; }
    if (s >= n_src - 1) { f = 0.0f; s = n_src - 1; }
    w1 = (int)rintf(f * 2048.0f);
    w0 = (int)rintf((1.0f - f) * 2048.0f);
    s0 = s;
    s1 = min(s + 1, n_src - 1);
}

__device__ __forceinline__ int crop_px(const CropK &p, int wx, int wy, int c)
{
    const int ix = p.x0 + wx, iy = p.y0 + wy;
    if ((unsigned)ix >= (unsigned)p.W || (unsigned)iy >= (unsigned)p.H) return p.fill[c];
    return p.im[((long)iy * p.W + ix) * 3 + c];
}

// output pixel (dx, dy), all three channels
__device__ __forceinline__ void crop_resize_px(const CropK &p, int dx, int dy)
{
    if (p.win == p.S) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p.out[((long)c * p.S + dy) * p.S + dx] = (float)crop_px(p, dx, dy, c);
        return;
    }
    if (p.win == 2 * p.S) {          // exact 2x downscale: cv2.resize switches INTER_LINEAR to INTER_AREA
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int v = (crop_px(p, 2 * dx, 2 * dy, c) + crop_px(p, 2 * dx + 1, 2 * dy, c) +
                           crop_px(p, 2 * dx, 2 * dy + 1, c) + crop_px(p, 2 * dx + 1, 2 * dy + 1, c) + 2) >> 2;
            p.out[((long)c * p.S + dy) * p.S + dx] = (float)v;
        }
        return;
    }
    int xa, xb, wxa, wxb, ya, yb, wya, wyb;
    crop_axis(dx, p.win, p.S, xa, xb, wxa, wxb);
    crop_axis(dy, p.win, p.S, ya, yb, wya, wyb);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long top = (long)crop_px(p, xa, ya, c) * wxa + (long)crop_px(p, xb, ya, c) * wxb;
        const long bot = (long)crop_px(p, xa, yb, c) * wxa + (long)crop_px(p, xb, yb, c) * wxb;
        long v = ((((long)wya * (top >> 4)) >> 16) + (((long)wyb * (bot >> 4)) >> 16) + 2) >> 2;
        v = v < 0 ? 0 : (v > 255 ? 255 : v);
        p.out[((long)c * p.S + dy) * p.S + dx] = (float)v;
    }
}

}  // namespace usot_head
