"""Lists, operands, float64 references and mutations of the correlation and RoI-pool sweep (tests/test_gpu_corr_pool_sweep.py, pinned by
tests/test_corr_pool_lists.py).  Host only: numpy and the two oracles.

A. Per-plane xcorr (csrc/xcorr.hip section 2, csrc/xcorr_grad.hip).  x, k and dout hold integers in [-3, 3] and the gradients' scale is
   a power of two: every partial sum is an integer far below 2^24, so float32 in any order equals float64.

B. Precise RoI Pooling (csrc/head_ops.hip).  The DYADIC FAMILY: features and top_diff are small integers, every bin edge is a multiple
   of 1/4 and every bin is 1/4, 1/2, 1, 2 or 4 wide and high.  Then each hat integral is a multiple of 1/32, each bin area a power of
   two, and every product and sum of the forward and of the feature gradient is a dyadic rational of a few bits: float32 == float64.
   The RoI gradient multiplies by pw / PW and is exact where PH and PW are powers of two."""
import functools

import numpy as np

import prroi_exact as ex

# ================================================================================================================== A. xcorr planes
TEMPLATES = ((5, 5), (3, 5), (5, 3))                 # the specialised kernels
XC_P = (1, 2, 3, 4, 5, 7, 8, 9, 17)
XC_P_WX = (31, 33)
XC_WX_LAST = 66
XC_ENTRIES = ('out', 'dx', 'dk')
PLANES_CAP = 4096 * 4                                # wavefronts of the largest plane-kernel grid
GENERIC_CAP = 8192 * 256                             # threads of the largest generic grid


def hx_list(hk):
    return (hk, hk + 1, hk + 6)


def wx_sweep(t):
    """(Hx, Wx, Hk, Wk, P): every Wx from Wk to 66 at Hx = Hk + 1 and 9 planes"""
    hk, wk = t
    return [(hk + 1, wx, hk, wk, 9) for wx in range(wk, XC_WX_LAST + 1)]


def p_sweep(t):
    hk, wk = t
    return [(hx, wx, hk, wk, p) for p in XC_P for wx in XC_P_WX for hx in hx_list(hk)]


XC_GENERIC = [(hx, wx, hk, wk, p)
              for (hk, wk), maps in (((1, 1), ((1, 1), (4, 7))), ((2, 4), ((2, 4), (5, 9))), ((7, 7), ((7, 7), (9, 12))),
                                     ((5, 5), ((5, 65), (6, 65), (11, 65))))
              for hx, wx in maps for p in (1, 3, 40)]

# past the grid caps, one problem per kernel family; big planes are gathered from XC_BASE_PLANES base planes
XC_BASE_PLANES = 64
XC_BIG = {
    'planes2': (5, 6, 5, 5, 2 * PLANES_CAP + 9),                 # two planes per wavefront
    'planes1': (5, 33, 5, 5, PLANES_CAP + 5),                    # one plane per wavefront
    'generic': (9, 12, 2, 4, 29131),                             # out 72 and dx 108 elements per plane
    'generic_dk': (12, 13, 12, 12, 14567),                       # dk 144 elements per plane
}
XC_BIG_ENTRIES = {'planes2': XC_ENTRIES, 'planes1': XC_ENTRIES, 'generic': ('out', 'dx'), 'generic_dk': ('dk',)}

# isolation: +Inf over every plane of one parity; the planes of the other parity stay exact
XC_ISOLATION = [(hk + 2, wx, hk, wk, p) for hk, wk in TEMPLATES for wx in (16, 32, 33) for p in (5, 6)]
XC_MUTATIONS = ['flip', 'shift', 'drop_col', 'dead_half', 'one_pass']


def xc_kernel(case):
    """which kernel the three launchers pick: 'planes2' (two planes per wavefront), 'planes1' or 'generic'"""
    hx, wx, hk, wk, p = case
    if (hk, wk) in TEMPLATES and wx <= 64:
        return 'planes2' if wx <= 32 else 'planes1'
    return 'generic'


def xc_counts(case):
    hx, wx, hk, wk, p = case
    return {'out': p * (hx - hk + 1) * (wx - wk + 1), 'dx': p * hx * wx, 'dk': p * hk * wk}


def xc_first_pass(case):
    """leading elements of each output that the first pass of the grid-stride loop writes"""
    hx, wx, hk, wk, p = case
    kern, n = xc_kernel(case), xc_counts(case)
    if kern == 'generic':
        return {e: min(n[e], GENERIC_CAP) for e in XC_ENTRIES}
    planes = min(p, PLANES_CAP * (2 if kern == 'planes2' else 1))
    return {e: n[e] // p * planes for e in XC_ENTRIES}


def xc_scale(case):
    return (0.5, 2.0, 0.25)[(case[1] + case[4]) % 3]


def xc_operands(case, seed=0):
    """x [P][Hx][Wx], k [P][Hk][Wk], dout [P][OH][OW]: float32 integers in [-3, 3]"""
    hx, wx, hk, wk, p = case
    g = np.random.default_rng([seed, hx, wx, hk, wk, p])
    return tuple(g.integers(-3, 4, s).astype(np.float32) for s in ((p, hx, wx), (p, hk, wk), (p, hx - hk + 1, wx - wk + 1)))


def xc_big_index(name, seed=0):
    """seeded plane index of a big problem into its base"""
    return np.random.default_rng([seed, XC_BIG[name][4]]).integers(0, XC_BASE_PLANES, XC_BIG[name][4])


def xc_base(name):
    return XC_BIG[name][:4] + (XC_BASE_PLANES,)


def xc_ref(x, k, dout, scale, mutate=None):
    """float64 {'out', 'dx', 'dk'} from the three formulas on top of csrc/xcorr_grad.hip:
         out[p][i][j] = sum_{u,v} x[p][i+u][j+v] k[p][u][v]
         dx[p][a][b]  = scale sum_{u,v} dout[p][a-u][b-v] k[p][u][v]
         dk[p][u][v]  = scale sum_{i,j} dout[p][i][j] x[p][i+u][j+v]
    mutate: 'flip' (a convolution: the template turned by 180 degrees), 'shift' (the window starts one column late), 'drop_col' (dout's
    last column is not read, out's not stored), 'dead_half' (with two planes per wavefront and an odd P the idle half works as plane P - 1
    and stores one plane behind the output: the result gains that plane), 'one_pass' (no second pass of the grid-stride loop: what it
    would write stays NaN)."""
    x, k, dout = (np.asarray(a, np.float64) for a in (x, k, dout))
    p, hx, wx = x.shape
    hk, wk = k.shape[1:]
    oh, ow = hx - hk + 1, wx - wk + 1
    assert dout.shape == (p, oh, ow)
    case = (hx, wx, hk, wk, p)
    if mutate == 'flip':
        k = k[:, ::-1, ::-1]
    if mutate == 'shift':
        x = np.concatenate([x[:, :, 1:], np.zeros((p, hx, 1))], 2)
    if mutate == 'drop_col':
        dout = dout.copy()
        dout[:, :, -1] = 0.0
    out, dx, dk = np.zeros((p, oh, ow)), np.zeros((p, hx, wx)), np.zeros((p, hk, wk))
    for u in range(hk):
        for v in range(wk):
            win = x[:, u:u + oh, v:v + ow]
            out += win * k[:, u, v][:, None, None]
            dx[:, u:u + oh, v:v + ow] += dout * k[:, u, v][:, None, None]
            dk[:, u, v] = (dout * win).sum((1, 2))
    if mutate == 'flip':
        dk = dk[:, ::-1, ::-1]                       # the taps of the turned template
    res = {'out': out, 'dx': dx * scale, 'dk': dk * scale}
    if mutate == 'drop_col':
        res['out'][:, :, -1] = np.nan
    if mutate == 'dead_half' and xc_kernel(case) == 'planes2' and p % 2:
        res = {e: np.concatenate([a, a[-1:]]) for e, a in res.items()}
    if mutate == 'one_pass':
        first = xc_first_pass(case)
        for e, a in res.items():
            a.reshape(-1)[first[e]:] = np.nan
    return res


# ======================================================================================================================= B. PrRoIPool
PR_MAP = (2, 4, 9, 11)                               # B, C, H, W
PR_BINS = (0.25, 0.5, 1.0, 2.0, 4.0)
PR_SHAPES = ((7, 7), (3, 5), (1, 1), (4, 8), (8, 8), (2, 1))
PR_SCALES = (1.0, 0.5)
PR_ROI_EXACT = ((1, 1), (4, 8), (8, 8), (2, 1))      # pw / PW and ph / PH dyadic: the RoI gradient is exact too
PR_ROI_BAR = 3e-5                                    # test_prroi_roi_gradient_vs_oracles' bar for bins of at least 0.2 pixel
PR_FWD_CAP = 4096 * 256
PR_COOR_CAP = 64 * 256
PR_MUTATIONS = ['floor_plus_1', 'cell_le', 'pixel_lt', 'clamp', 'roi_area', 'scale_width', 'fx1']


def pr_starts():
    B, C, H, W = PR_MAP
    return (-2.25, -1.0, 0.0, 0.5, 3.75, W - 2.0, W - 1.0, W - 0.25, W + 1.0), (-1.5, 0.0, 2.25, H - 1.0)


# degenerate boxes in feature coordinates: zero width, zero height, negative width, negative height, outside on either side
PR_EXTRAS = ((3.0, 2.0, 3.0, 6.0), (2.0, 4.0, 7.0, 4.0), (6.0, 5.0, 4.0, 8.0), (1.0, 7.5, 5.0, 2.5), (20.0, 20.0, 24.0, 26.0),
             (-9.0, -9.0, -5.0, -3.0))


def pr_rois(ph, pw, scale):
    """[R][5] float32 (batch, x1, y1, x2, y2): bin width x start x x start y, the bin height walking through PR_BINS against the width,
    the batch index alternating; then PR_EXTRAS.  Coordinates are given in feature pixels and divided by the scale (a power of two)."""
    sx, sy = pr_starts()
    rows = []
    for a, bw in enumerate(PR_BINS):
        for b, x0 in enumerate(sx):
            for c, y0 in enumerate(sy):
                bh = PR_BINS[(a + b + c) % len(PR_BINS)]
                rows.append((len(rows) % 2, x0, y0, x0 + bw * pw, y0 + bh * ph))
    for e in PR_EXTRAS:
        rows.append((len(rows) % 2,) + e)
    r = np.array(rows, np.float64)
    r[:, 1:] /= scale
    assert np.array_equal(r, r.astype(np.float32))
    return r.astype(np.float32)


def pr_features(C=None, B=None, seed=0):
    b, c, H, W = PR_MAP
    return np.random.default_rng([seed, 1]).integers(-4, 5, (B or b, C or c, H, W)).astype(np.float32)


def pr_top_diff(R, ph, pw, C=None, seed=0):
    return np.random.default_rng([seed, 2, R, ph, pw]).integers(-3, 4, (R, C or PR_MAP[1], ph, pw)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pr_case(ph, pw, scale):
    """one list with its operands and float64 expectations (computed once per process)"""
    rois, f = pr_rois(ph, pw, scale), pr_features()
    g = pr_top_diff(len(rois), ph, pw)
    d = dict(rois=rois, f=f, g=g, out=ex.prroi_pool_exact(f, rois, ph, pw, scale),
             gin=ex.prroi_pool_exact_backward(f.shape, rois, g, ph, pw, scale),
             groi=ex.prroi_pool_exact_coor_backward(f, rois, g, ph, pw, scale))
    for a in d.values():
        a.setflags(write=False)
    return d


def pr_geometry(roi, ph, pw, scale, mutate=None):
    s = float(np.float32(scale))
    x1, y1, x2, y2 = (float(np.float32(v)) for v in roi[1:])
    if mutate == 'scale_width':
        rsw, rsh, rew, reh = x1, y1, x1 + (x2 - x1) * s, y1 + (y2 - y1) * s
    else:
        rsw, rsh, rew, reh = x1 * s, y1 * s, x2 * s, y2 * s
    rw, rh = max(rew - rsw, 0.0), max(reh - rsh, 0.0)
    return rsw, rsh, rw / pw, rh / ph, rw, rh


def _piece(a, b):
    """integral of 1 - t over [a, b]"""
    return b - 0.5 * b * b - a + 0.5 * a * a


def pr_axis(lo, hi, n, mutate=None, pixels=False):
    """The hat integrals of one bin along one axis, assembled cell by cell as csrc/head_ops.hip does: {pixel: weight} over the
    unit cells floor(lo) .. ceil(hi) - 1, each giving its near and its far corner a piece.  pixels=True is the feature gradient's form:
    a loop over the pixels s .. e clipped to the map.  Pixels outside 0 .. n - 1 are kept (the caller zero-extends or clamps)."""
    s = int(np.floor(lo))
    e = int(np.floor(hi)) + 1 if mutate == 'floor_plus_1' else int(np.ceil(hi))
    w = {}
    if pixels:
        last = e - 1 if mutate == 'pixel_lt' else e
        for i in range(max(s, 0), min(last, n - 1) + 1):
            v = 0.0
            if i > s:
                v += _piece(i - min(hi, i), i - max(lo, i - 1))
            if i < e:
                v += _piece(max(lo, i) - i, min(hi, i + 1) - i)
            w[i] = v
        return w
    for c in range(s, e + 1 if mutate == 'cell_le' else e):
        a, b = max(lo, c), min(hi, c + 1)
        w[c] = w.get(c, 0.0) + _piece(a - c, b - c)
        w[c + 1] = w.get(c + 1, 0.0) + _piece(c + 1 - b, c + 1 - a)
    return w


def _taps(fb, wy, wx, mutate):
    """sum_{y,x} wy[y] wx[x] f[:, y, x] over a zero-extended (mutate 'clamp': edge-replicated) map -> [C]"""
    C, H, W = fb.shape
    acc = np.zeros(C)
    for y, a in wy.items():
        if mutate == 'clamp':
            y = min(max(y, 0), H - 1)
        elif not 0 <= y < H:
            continue
        for x, b in wx.items():
            if mutate == 'clamp':
                x = min(max(x, 0), W - 1)
            elif not 0 <= x < W:
                continue
            acc += (a * b) * fb[:, y, x]
    return acc


def pr_forward_cells(f, rois, ph, pw, scale, mutate=None):
    """float64 restatement of prroi_forward_kernel's cell loop, with the listed mutations"""
    f = np.asarray(f, np.float64)
    out = np.zeros((len(rois), f.shape[1], ph, pw))
    for r, roi in enumerate(rois):
        x0, y0, bw, bh, rw, rh = pr_geometry(roi, ph, pw, scale, mutate)
        if not bw * bh > 0.0:
            continue
        div = rw * rh if mutate == 'roi_area' else bw * bh
        for i in range(ph):
            wy = pr_axis(y0 + bh * i, y0 + bh * i + bh, f.shape[2], mutate)
            for j in range(pw):
                wx = pr_axis(x0 + bw * j, x0 + bw * j + bw, f.shape[3], mutate)
                out[r, :, i, j] = _taps(f[int(roi[0])], wy, wx, mutate) / div
    return out


def pr_backward_terms(shape, rois, g, ph, pw, scale, mutate=None, g_abs=None):
    """float64 restatement of prroi_backward_kernel's pixel loop.  Returns (gradient, sum of |terms| per element, the finest power of
    two dividing any term of the element): every term is one atomicAdd of the kernel.  g_abs: sum of |top_diff| where g is itself a
    sum over several RoIs (the gathered list)."""
    B, C, H, W = shape
    g = np.asarray(g, np.float64)
    g_abs = np.abs(g) if g_abs is None else np.asarray(g_abs, np.float64)
    out, mag, quantum = np.zeros(shape), np.zeros(shape), np.full(shape, np.inf)
    for r, roi in enumerate(rois):
        b = int(roi[0])
        x0, y0, bw, bh, rw, rh = pr_geometry(roi, ph, pw, scale, mutate)
        if not bw * bh > 0.0 or not 0 <= b < B:
            continue
        div = rw * rh if mutate == 'roi_area' else bw * bh
        for i in range(ph):
            wy = pr_axis(y0 + bh * i, y0 + bh * i + bh, H, mutate, pixels=True)
            for j in range(pw):
                wx = pr_axis(x0 + bw * j, x0 + bw * j + bw, W, mutate, pixels=True)
                if not wy or not wx:
                    continue
                ys, xs = sorted(wy), sorted(wx)
                o = np.outer([wy[y] for y in ys], [wx[x] for x in xs]) / div
                sl = (b, slice(None), slice(ys[0], ys[-1] + 1), slice(xs[0], xs[-1] + 1))
                out[sl] += g[r, :, i, j][:, None, None] * o
                t = g_abs[r, :, i, j][:, None, None] * o
                mag[sl] += t
                if mutate is None:
                    quantum[sl] = np.minimum(quantum[sl], lowest_bit(t))
    return out, mag, quantum


def lowest_bit(t):
    """the largest power of two dividing each element of a dyadic array (inf for 0)"""
    n = np.abs(t) * 2.0 ** 40
    k = n.astype(np.int64)
    assert np.array_equal(k, n), 'not a multiple of 2^-40'
    return np.where(k == 0, np.inf, (k & -k).astype(np.float64) * 2.0 ** -40)


def pr_coor_terms(f, rois, g, ph, pw, scale, mutate=None):
    """float64 restatement of prroi_coor_backward_kernel: [R][C][PH][PW][4] contributions to (x1, y1, x2, y2), one per pooled
    element; a row of the RoI gradient is their sum in whatever order the wavefronts' atomics land"""
    f = np.asarray(f, np.float64)
    g = np.asarray(g, np.float64)
    B, C, H, W = f.shape
    s = float(np.float32(scale))
    ii, jj = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    terms = np.zeros((len(rois), C, ph, pw, 4))
    for r, roi in enumerate(rois):
        b = int(roi[0])
        x1, y1, bw, bh, rw, rh = pr_geometry(roi, ph, pw, scale)
        area = bw * bh
        if not area > 0.0 or not 0 <= b < B:
            continue
        for i in range(ph):
            ys, ye = y1 + i * bh, y1 + (i + 1) * bh
            hy = ex.hat_integrals(ys, ye, H)
            rows = np.tensordot(f[b], hy, axes=([1], [0]))                 # [C][W]
            for j in range(pw):
                xs, xe = x1 + j * bw, x1 + (j + 1) * bw
                hx = ex.hat_integrals(xs, xe, W)
                cols = f[b] @ hx                                            # [C][H]
                out = rows @ hx / area
                k = s / area * g[r, :, i, j]
                dxs, dxe = (-(rows @ ex._hat(xs - ii)) + bh * out) * k, (rows @ ex._hat(xe - ii) - bh * out) * k
                dys, dye = (-(cols @ ex._hat(ys - jj)) + bw * out) * k, (cols @ ex._hat(ye - jj) - bw * out) * k
                fx0, fx1, fy0, fy1 = j / pw, (j + 1) / pw, i / ph, (i + 1) / ph
                if mutate == 'fx1':
                    fx1 = fx0
                terms[r, :, i, j] = np.stack([dxs * (1 - fx0) + dxe * (1 - fx1), dys * (1 - fy0) + dye * (1 - fy1),
                                              dxs * fx0 + dxe * fx1, dys * fy0 + dye * fy1], 1)
    return terms


def pr_alignment(rois, ph, pw, scale):
    """how many bins of a list reach each alignment class, per axis: a left edge on a pixel, a right edge on a pixel, a bin inside one
    unit cell, and edges at -1, 0, n - 1 and n"""
    B, C, H, W = PR_MAP
    c = {}

    def hit(key, n=1):
        c[key] = c.get(key, 0) + n

    for roi in rois:
        x0, y0, bw, bh, rw, rh = pr_geometry(roi, ph, pw, scale)
        if not bw * bh > 0.0:
            continue
        for axis, lo0, step, n, count, other in (('x', x0, bw, W, pw, ph), ('y', y0, bh, H, ph, pw)):
            for q in range(count):
                lo, hi = lo0 + step * q, lo0 + step * q + step
                if np.floor(lo) == lo:
                    hit(axis + ' left aligned', other)
                if np.ceil(hi) == hi:
                    hit(axis + ' right aligned', other)
                if np.ceil(hi) - np.floor(lo) == 1:
                    hit(axis + ' one cell', other)
                for e in (lo, hi):
                    for name, v in (('-1', -1), ('0', 0), ('n-1', n - 1), ('n', n)):
                        if e == v:
                            hit('%s edge at %s' % (axis, name), other)
    return c


# ---- past the grid caps ----------------------------------------------------------------------------------------------------------
PR_BIG_BASE = 64
PR_BIG_R = PR_FWD_CAP // (PR_MAP[1] * 49) + 2        # 5351 RoIs of 4 x 7 x 7: 1 048 796 pooled elements
PR_BIG_SHAPE = (7, 7)


def pr_big_base():
    """64 RoIs of the 7 x 7 list at scale 1: every third of the 180 regular ones, then four of the extras"""
    rois = pr_rois(7, 7, 1.0)
    pick = list(range(0, 180, 3)) + list(range(180, 184))
    return rois[pick]


def pr_big_index(seed=0):
    return np.random.default_rng([seed, PR_BIG_R]).integers(0, PR_BIG_BASE, PR_BIG_R)


def pr_big_top_diff(seed=0):
    """integers in [-1, 1]: some 84 copies of a base RoI add up on one pixel, and with [-3, 3] the sum of |terms| over the finest power
    of two would pass 2^24 (1.19 of it; 0.59 here, asserted by tests/test_corr_pool_lists.py)"""
    return np.random.default_rng([seed, 5, PR_BIG_R]).integers(-1, 2, (PR_BIG_R, PR_MAP[1], 7, 7)).astype(np.float32)


def pr_big_summed(idx, g):
    """top_diff summed per base RoI, and the sum of its magnitudes"""
    tot, mag = np.zeros((PR_BIG_BASE,) + g.shape[1:]), np.zeros((PR_BIG_BASE,) + g.shape[1:])
    np.add.at(tot, idx, g.astype(np.float64))
    np.add.at(mag, idx, np.abs(g.astype(np.float64)))
    return tot, mag


PR_WIDE_C = 260                                      # 260 x 8 x 8 = 16 640 elements per RoI: two passes of the 64-block grid
PR_WIDE_ROIS = np.array([[0, 0.5, 0.0, 8.5, 16.0], [0, 3.0, -1.0, 11.0, 7.0], [0, -1.0, 2.0, 15.0, 10.0]], np.float32)
PR_MAX_R = 65535


def pr_unit_rows(ph=1, pw=1, scale=1.0):
    """RoI gradient of each RoI of the 1 x 1 list on channel 0 alone with top_diff 1 (the operator is linear in top_diff)"""
    c = pr_case(ph, pw, scale)
    return ex.prroi_pool_exact_coor_backward(c['f'][:, :1], c['rois'], np.ones((len(c['rois']), 1, ph, pw)), ph, pw, scale)


# the forward with +Inf one pixel past an aligned right / lower edge: a kernel that walks one cell too far multiplies it by 0
PR_INF_ROIS = np.array([[0, 1.0, 1.0, 5.0, 5.0], [1, 0.5, 2.25, 4.5, 4.25], [0, 3.0, 1.0, 5.0, 5.0]], np.float32)
PR_INF_SHAPE = (2, 4)


def pr_inf_features():
    f = pr_features().copy()
    f[:, :, :, 6] = np.inf                            # every RoI ends at x = 5 or 4.5: column 6 is never under a hat
    f[:, :, 6, :] = np.inf                            # and at y = 5 or 4.25
    return f
