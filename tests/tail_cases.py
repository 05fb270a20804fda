"""Shared by test_tail_lists.py and test_gpu_tail_sweep.py: the case lists, seeded operands and references of the frame-tail sweep -
the kernels that open and close a frame (csrc/head_ops.hip, head_common.h, multitrack.hip): decode (usot_decode_f32 / _dev_f32 /
_batch_f32), the thin 3x3 heads (usot_thin_conv3x3_f32), the crop (usot_crop_resize_u8_f32 and its batch), the Conf_Fusion reduction
(usot_conf_fusion_reduce_f32 / _lp / _map_f32), the movers (usot_permute4_f32, usot_rows_copy_f32, usot_rows_copy_multi_f32) and the
lock-step append + gather (usot_rows_append_gather_batch_f32).

The references are written from the operator definitions of include/usot_hip.h and the reference tracker lines cited there, in
float64 NumPy / torch-CPU (integers for the crop); nothing here imports the engine's launch logic.  Where a test has to know WHICH
path a launch takes (thin_plan) the launcher's documented rule is restated, so that the lists can be asserted to reach every path.

Why the comparisons are equalities:
  decode   bbox values are multiples of 1/4 in [4, 60] and the grid is integer: gx -+ b, the box edges and w, h are exact in float64.
           A planted winner has logits +12 in both maps and the target's box, so its penalty is exp(-0) = 1 exactly and its pscore
           0.679 s + 0.321 window with s = sigmoid(12) - every other cell has logits <= 0, pscore <= 0.3395 + 0.321 window: the winner
           leads by >= 0.018 even in a window corner (asserted: >= 1e-4 on every non-tie case).  sigmoid(12) in float32 is 51.54 ulp
           of 1.0 above 1, 0.04 ulp from the nearest rounding boundary and 1e4 times further than any expf error, and the blend
           0.3 s + 0.7 s rounds alike with and without a fused multiply-add (asserted), so the winner's score is bit-stable.
           Ties come from bit-identical inputs (window_influence 0, or two mirrored cells of the bitwise symmetric Hanning window).
  thin     x multiples of 1/4 with |x| <= 4, w multiples of 1/4 with |w| <= 1, biases multiples of 1/4: every partial sum in any order
           is a multiple of 1/16 below 2^24 / 16 (asserted) - ACT_NONE / ACT_RELU outputs equal float64 bit for bit, and under
           ACT_EXP / ACT_CONF the pre-activation is exact, the device's expf the only error.
  expf     torch-CPU float32 exp against float64 exp on the sweep's own arguments: max relative error EXP_CPU_ERR = 5.11e-8
           (measured; asserted by the list test).  The device function need not be correctly rounded: EXP_ALLOW = 4 x that = 2.04e-7.
  crop     integer arithmetic: hostutils.get_subwindow_tracking + resize_bilinear_u8 (OpenCV's fixed-point rule restated).
  reduce   confidences are powers of two whose sum over the slots is a power of two, values multiples of 1/4 with |v| <= 63.75 (exact
           in fp16 and bf16 too): c / den and every product and partial sum are exact, a 16-bit output is the round-to-nearest-even.

Plain helper module."""
import collections
import functools
import itertools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
CANARY32 = 0x7FC17FC1                                  # tests/guarded.py's pattern as a float32 word


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# =========================================================================================================================== decode
STRIDE, RATIO, PENALTY_K, WINDOW_INFLUENCE = 8, 0.3, 0.021, 0.321
PLANT = 12.0                                           # a planted winner's logit in both maps
TARGET_BOX = (18.0, 14.0, 18.0, 14.0)                  # its box: w = tw = 36, h = th = 28
FAR = 4096.0                                           # a clamp case's box: 4096 px beyond the cell, every RoI clamp fires
NAN_KINDS = ['nan_cls', 'nan_mem', 'nan_box']
DEC_KINDS = ['win', 'tie'] + NAN_KINDS + ['all_nan', 'clamp_out', 'clamp_flip']
DEC_MUTATIONS = ['argmax_last', 'argmax_thread', 'clamp_no_gap']

Dec = collections.namedtuple('Dec', 'S kind cells wi')  # cells: where the kind plants; wi: the launch's window_influence


def instance_size(S):
    """the crop size whose response map is S wide (usot_tracker.py:366-394: S = (size - 127) / 8 + 9)"""
    return 127 + STRIDE * (S - 9)


def window(S):
    return np.outer(np.hanning(S), np.hanning(S)).reshape(-1)


def placements(S):
    """cell 0, the last cell, the last lane of wave 0, the first lane of wave 1, cell 1023 and - from S = 33, where a thread owns
    several cells - cell 1024"""
    n = S * S
    return sorted({c for c in (0, n - 1, 63, 64, 1023, 1024) if c < n})


def tie_pairs(S):
    """(first, second, window_influence).  At window_influence 0: first / last cell, two cells of one wave, of two waves, of one
    thread on two passes (i, i + 1024), and a later cell owned by a LOWER thread (1000, 1029).  At the project's window_influence two
    mirrored cells of the window: an interior pair and, from S = 33, a same-thread pair (odd S) and a lower-thread pair."""
    n = S * S
    out = [(a, b, 0.0) for a, b in ((0, n - 1), (3, 40), (10, 100), (5, 1029), (1000, 1029)) if a < b < n]
    a = S + 1 if S >= 3 else 0
    mirrored = [(a, n - 1 - a)]
    if n > 1025:
        if n % 2:
            mirrored.append(((n - 1025) // 2, (n - 1025) // 2 + 1024))
        a = (n - 1025) // 2 + 8
        mirrored.append((a, n - 1 - a))
    return out + [(a, b, WINDOW_INFLUENCE) for a, b in mirrored if a < b < n]


@functools.lru_cache(maxsize=None)
def decode_cases(S):
    n = S * S
    cases = [Dec(S, 'win', (c,), WINDOW_INFLUENCE) for c in placements(S)]
    cases += [Dec(S, 'tie', (a, b), wi) for a, b, wi in tie_pairs(S)]
    for kind in NAN_KINDS:
        cases += [Dec(S, kind, (c,), WINDOW_INFLUENCE) for c in placements(S)]
        cases += [Dec(S, kind, (a, b), WINDOW_INFLUENCE) for a, b, wi in tie_pairs(S) if wi == 0.0]
    cases += [Dec(S, 'all_nan', (), WINDOW_INFLUENCE), Dec(S, 'clamp_out', (n // 2,), WINDOW_INFLUENCE),
              Dec(S, 'clamp_flip', (n // 2,), WINDOW_INFLUENCE)]
    return cases


DEC_S_F32 = list(range(1, 65))
DEC_S_DEV = list(range(2, 65))                         # at S = 1 the RoI slope is 0 / 0 in the reference as well
DEC_S_BATCH = list(range(2, 33))
DEC_BATCH_B = [1, 5]


@functools.lru_cache(maxsize=None)
def _decode_base(S):
    g, n = _rng('decode', S), S * S
    cls = (-g.integers(0, 25, n) / 4).astype(np.float32)                  # <= 0
    cm = (-g.integers(0, 25, n) / 4).astype(np.float32)
    bbox = (g.integers(16, 241, (4, n)) / 4).astype(np.float32)           # multiples of 1/4 in [4, 60]
    return cls, cm, bbox


def decode_operands(case):
    """-> cls [n], cls_mem [n], bbox [4, n] (float32), tw, th"""
    cls, cm, bbox = (a.copy() for a in _decode_base(case.S))
    n = case.S * case.S
    tw, th = TARGET_BOX[0] + TARGET_BOX[2], TARGET_BOX[1] + TARGET_BOX[3]

    def plant(c, box=TARGET_BOX):
        cls[c] = cm[c] = PLANT
        bbox[:, c] = box
    if case.kind in ('win', 'tie'):
        for c in case.cells:
            plant(c)
    elif case.kind in NAN_KINDS:
        rest = [c for c in range(n) if c not in case.cells]
        if rest:                                                          # a finite winner that must lose to the NaN
            plant(rest[len(rest) // 2])
        for c in case.cells:
            if case.kind == 'nan_cls':
                cls[c] = np.nan
            elif case.kind == 'nan_mem':
                cm[c] = np.nan
            else:
                bbox[case.cells[0] % 4, c] = np.nan                       # one coordinate: the other three stay finite
    elif case.kind == 'all_nan':
        cls[:], cm[:], bbox[:] = np.nan, np.nan, np.nan
    else:
        far = FAR if case.kind == 'clamp_out' else -FAR
        plant(case.cells[0], (far,) * 4)
        tw = th = 2 * FAR
    return cls, cm, bbox, tw, th


def _argmax(ps, mut=None):
    nan = np.isnan(ps)
    cand = np.flatnonzero(nan) if nan.any() else np.flatnonzero(ps == ps.max())
    if mut == 'argmax_last':                                              # keeps the last maximum
        return int(cand[-1])
    if mut == 'argmax_thread':                                            # orders by the owning thread (cell mod 1024), then cell
        return int(min(cand, key=lambda i: (i % 1024, i)))
    return int(cand[0])


def roi_ref(box, S, instance_size, stride, mut=None):
    """pool_label_search (usot_tracker.py:329-350): the box rounded to float32, clamped one grid gap outside the S-point axis,
    mapped to feature coordinates in float64, stored as float32.  np.clip keeps a NaN."""
    lo = float((0 - S // 2) * stride + instance_size // 2)
    hi = float((S - 1 - S // 2) * stride + instance_size // 2)
    slope = 2 * (S // 2) / (hi - lo)
    gap = 0.0 if mut == 'clamp_no_gap' else 1.0 / slope
    v = np.asarray(box, np.float32).astype(np.float64)
    return ((np.clip(v, lo - gap, hi + gap) - lo) * slope).astype(np.float32)


def decode_ref(cls, cls_mem, bbox, window, S, instance_size, stride, ratio, penalty_k, window_influence, tw, th, mut=None):
    """usot_tracker.py:138-163: float32 sigmoid and blend, everything behind it in float64, np.argmax (the first maximum wins, the
    first NaN wins) -> dict(i, sc, pen, box [4], ps, roi [4], pscore [n])"""
    f = np.float32
    with np.errstate(all='ignore'):
        sig = lambda a: (f(1) / (f(1) + np.exp(-a.astype(f)))).astype(f)
        sc = (f(ratio) * sig(cls) + (f(1) - f(ratio)) * sig(cls_mem)).astype(f)
        ax = ((np.arange(S) - S // 2) * stride + instance_size // 2).astype(np.float64)
        gx, gy = np.tile(ax, S), np.repeat(ax, S)
        b = bbox.astype(np.float64)
        x1, y1, x2, y2 = gx - b[0], gy - b[1], gx + b[2], gy + b[3]
        w, h = x2 - x1, y2 - y1
        size = lambda w_, h_: np.sqrt((w_ + (w_ + h_) * 0.5) * (h_ + (w_ + h_) * 0.5))
        sr = size(w, h) / size(tw, th)
        sr = np.maximum(sr, 1.0 / sr)
        rr = (tw / th) / (w / h)
        rr = np.maximum(rr, 1.0 / rr)
        pen = np.exp(-(rr * sr - 1.0) * penalty_k)
        ps = pen * sc.astype(np.float64) * (1.0 - window_influence) + window * window_influence
        i = _argmax(ps, mut)
        assert mut is not None or i == int(np.argmax(ps))
        box = np.array([x1[i], y1[i], x2[i], y2[i]])
        roi = roi_ref(box, S, instance_size, stride, mut) if S > 1 else None
    return dict(i=i, sc=sc[i], pen=pen[i], box=box, ps=ps[i], roi=roi, pscore=ps)


def decode_expected(case, mut=None):
    cls, cm, bbox, tw, th = decode_operands(case)
    S = case.S
    return decode_ref(cls, cm, bbox, window(S), S, instance_size(S), STRIDE, RATIO, PENALTY_K, case.wi, tw, th, mut)


def decode_margin(case, ref):
    """the winner's lead over the best cell that is not planted to tie with it (finite cases)"""
    ps = ref['pscore'].copy()
    ps[list(case.cells)] = -np.inf
    return float(ref['ps'] - ps.max()) if ps.size > len(case.cells) else np.inf


DEC_REFUSALS = {
    'f32': ['S0', 'S65', 'cls0', 'cls_mem0', 'bbox0', 'window0', 'out0'],
    'dev': ['S0', 'S65', 'cls0', 'cls_mem0', 'bbox0', 'window0', 'out0', 'tsz0'],
    'batch': ['S0', 'S33', 'B0', 'B65536', 'cls0', 'cls_mem0', 'bbox0', 'window0', 'out0', 'ctl0', 'roi0'],
}


# ================================================================================================================== thin 3x3 heads
ACT_NONE, ACT_RELU, ACT_EXP, ACT_CONF = 0, 1, 2, 3
EXACT_ACTS = (ACT_NONE, ACT_RELU)
EXP_CPU_ERR = 5.11e-8                                  # torch-CPU float32 exp vs float64 exp on the sweep's arguments (measured)
EXP_ALLOW = 4 * EXP_CPU_ERR
CONF_EDGES = [-1 / 16, 0.0, 1 / 16, 63 / 16, 4.0, 65 / 16]
TAPS = [(0, 0), (0, 2), (2, 0), (2, 2), (1, 1)]
FAMILIES = ['neg', 'pos', 'mixed', 'tap']
THIN_MUTATIONS = ['pad_row', 'row_lane']
THIN_N = 3                                             # images of a per-pixel case

Prob = collections.namedtuple('Prob', 'cout act groups bias pad')     # bias: False = a null pointer; pad: padded group strides
Thin = collections.namedtuple('Thin', 'N H W Cin probs share')       # share: every problem reads the same activations


def P(cout, act=ACT_NONE, groups=1, bias=True, pad=False):
    return Prob(cout, act, groups, bias, pad)


THIN_CIN = [4, 64, 252, 256, 260, 512]
THIN_HW = [(1, 1), (1, 5), (5, 1), (3, 4), (7, 7)]
THIN_ACTS = [ACT_NONE, ACT_RELU, ACT_EXP, ACT_CONF]


def thin_pixel_cases(cin):
    """one problem: every Cout, shape and activation at this Cin"""
    return [Thin(THIN_N, h, w, cin, (P(co, act),), False) for co in range(1, 5) for h, w in THIN_HW for act in THIN_ACTS]


def thin_multi_cases():
    """1..4 problems with mixed Cout, groups 1..3 with padded strides, null biases"""
    out = []
    for cin, (h, w) in ((4, (3, 4)), (256, (7, 7)), (260, (1, 5)), (512, (5, 1))):
        out += [Thin(THIN_N, h, w, cin, (P(4, ACT_EXP), P(1, ACT_NONE, 2, pad=True)), False),             # the frame's launch
                Thin(THIN_N, h, w, cin, (P(1, ACT_RELU), P(2, ACT_CONF), P(3, ACT_NONE)), False),
                Thin(THIN_N, h, w, cin, (P(4, ACT_NONE), P(3, ACT_RELU), P(2, ACT_EXP), P(1, ACT_CONF)), False),
                Thin(THIN_N, h, w, cin, (P(1), P(1, ACT_RELU, bias=False), P(1, ACT_EXP, bias=False), P(1, ACT_CONF, bias=False)), False),
                Thin(THIN_N, h, w, cin, (P(2, ACT_NONE, 3, pad=True), P(3, ACT_RELU, 2, pad=True)), False),
                Thin(THIN_N, h, w, cin, (P(4, ACT_RELU, 3, bias=False, pad=True),), False),
                Thin(THIN_N, h, w, cin, (P(2, ACT_CONF, 2, pad=True), P(4, ACT_NONE, 1, bias=False)), False)]
    return out


ROW_W = [1, 2, 25, 63, 64]


def thin_row_cases(W):
    """Cin 256 and >= 1024 rows: the wavefront-per-row form.  Three problems of each Cout on shared activations (43 x 8 x 3 = 1032
    rows; with Cout 4 only the first is split: the launch then holds four)."""
    k = ROW_W.index(W)
    return [Thin(43, 8, W, 256, tuple(P(co, THIN_ACTS[(co + j + k) % 4]) for j in range(3)), True) for co in range(1, 5)]


def thin_split_cases():
    """(case, form, split problems, why)"""
    return [(Thin(128, 8, 2, 256, (P(4, ACT_EXP),), False), 'row', [0], 'a single 4-channel problem: split'),
            (Thin(128, 8, 25, 256, (P(4, ACT_NONE),), False), 'row', [0], 'a single 4-channel problem: split'),
            (Thin(43, 8, 25, 256, (P(4, ACT_NONE), P(4, ACT_EXP), P(1, ACT_RELU)), True), 'row', [0],
             'two 4-channel problems among three: only the first is split'),
            (Thin(32, 8, 25, 256, (P(4, ACT_RELU), P(1, ACT_CONF), P(1), P(1, ACT_EXP, bias=False)), True), 'row', [],
             'four problems, one of 4 channels: none is split'),
            (Thin(64, 8, 25, 256, (P(4, ACT_NONE, 2, pad=True),), False), 'row', [], '4 channels in two groups: not split'),
            (Thin(43, 8, 65, 256, (P(1, ACT_RELU), P(2, ACT_NONE), P(4, ACT_EXP)), True), 'pixel', [], 'W = 65: per pixel'),
            (Thin(1023, 1, 25, 256, (P(2, ACT_NONE),), False), 'pixel', [], '1023 rows: per pixel'),
            (Thin(1024, 1, 25, 256, (P(2, ACT_NONE),), False), 'row', [], '1024 rows: per row')]


def thin_plan(case, tile=0):
    """the launcher's documented rule (head_ops.hip: usot_thin_conv3x3_f32) -> ('row' | 'pixel', indices of the split problems)"""
    rows = sum(p.groups * case.N * case.H for p in case.probs)
    if not (case.Cin == 256 and case.W <= 64 and rows >= 1024 and tile != 70):
        return 'pixel', []
    n, split = len(case.probs), []
    for i, p in enumerate(case.probs):
        if n < 4 and p.cout == 4 and p.groups == 1:
            split.append(i)
            n += 1
    return 'row', split


def _family(case, pi, g, c):
    return FAMILIES[(pi + g + c) % 4]


def _filters(case, pi):
    """-> w [G, Cout, Cin, 3, 3], b [G, Cout] (float64 tensors of multiples of 1/4)"""
    p, cin = case.probs[pi], case.Cin
    rg = _rng('thin-w', case.Cin, case.H, case.W, pi, tuple(p))
    w = np.zeros((p.groups, p.cout, cin, 3, 3))
    b = np.zeros((p.groups, p.cout))
    for g in range(p.groups):
        for c in range(p.cout):
            if p.act == ACT_CONF:                      # the centre tap of one channel: pre = x / 4 + {0, 4} at the planted pixels
                w[g, c, (4 * c + 1) % cin, 1, 1] = 0.25
                b[g, c] = 4.0 * ((pi + g + c) % 2)
                if c >= 2:
                    w[g, c, (4 * c + 2) % cin, 0, 0] = 0.5
            elif p.act == ACT_EXP:                     # 1..3 taps: |pre| <= 8
                for _ in range(1 + c % 3):
                    w[g, c, rg.integers(cin), rg.integers(3), rg.integers(3)] = rg.choice([-0.5, -0.25, 0.25, 0.5])
                b[g, c] = rg.integers(-8, 9) / 4
            else:
                fam = _family(case, pi, g, c)
                if fam == 'neg':                       # grows with every real pixel that goes missing, stays above 0
                    w[g, c] = -rg.integers(1, 3, (cin, 3, 3)) / 4
                    b[g, c] = 18 * cin + 4
                elif fam == 'pos':
                    w[g, c] = rg.integers(1, 5, (cin, 3, 3)) / 4
                    b[g, c] = rg.integers(-8, 9) / 4
                elif fam == 'mixed':
                    w[g, c] = rg.integers(-4, 5, (cin, 3, 3)) / 4
                    b[g, c] = rg.integers(-2048, 2049) / 4
                else:                                  # the input at a known offset plus 32
                    kh, kw = TAPS[(pi + g + c + case.H + case.W) % 5]
                    w[g, c, rg.integers(cin), kh, kw] = 1.0
                    b[g, c] = 32.0
    if not p.bias:
        b[:] = 0.0
    return torch.from_numpy(w), torch.from_numpy(b)


def _conf_plants(case):
    """(n, h, w) of the three planted pixels: pixels 0..2 of image 0, or pixel 0 of images 0..2 on a smaller map"""
    if case.H * case.W >= 3:
        return [(0, k // case.W, k % case.W) for k in range(3)]
    return [(n, 0, 0) for n in range(3)]


def _activations(case, pi):
    """x [G, N, H, W, Cin] float64 tensor of multiples of 1/4 in [-4, 4]"""
    p = case.probs[pi]
    key = ('thin-x', case.N, case.H, case.W, case.Cin) + (() if case.share else (pi, tuple(p)))
    x = torch.from_numpy(_rng(*key).integers(-16, 17, (p.groups, case.N, case.H, case.W, case.Cin)) / 4)
    for q in (case.probs if case.share else [p]):
        if q.act == ACT_CONF:
            for c in range(q.cout):
                for (n, h, w), v in zip(_conf_plants(case), (-0.25, 0.0, 0.25)):
                    x[:, n, h, w, (4 * c + 1) % case.Cin] = v
    return x


def thin_strides(case, pi):
    """-> x_gs, w_gs, b_gs, y_gs in elements (padded where the problem asks for it)"""
    p = case.probs[pi]
    pad = 1 if p.pad else 0
    return (case.N * case.H * case.W * case.Cin + 8 * pad, p.cout * 9 * case.Cin + 4 * pad, p.cout + pad,
            case.N * p.cout * case.H * case.W + 3 * pad)


def _padded(rows, stride):
    """[G, len] -> flat float32 [G * stride], NaN in the gaps"""
    out = torch.full((rows.shape[0], stride), float('nan'), dtype=torch.float32)
    out[:, :rows.shape[1]] = rows.float()
    return out.reshape(-1)


@functools.lru_cache(maxsize=8)
def thin_build(case):
    """-> per problem dict(x, w, b: flat float32 device layouts (b None for a null bias), pre: float64 [G, N, Cout, H, W])"""
    out = []
    for pi, p in enumerate(case.probs):
        x, (w, b) = _activations(case, pi), _filters(case, pi)
        x_gs, w_gs, b_gs, y_gs = thin_strides(case, pi)
        G = p.groups
        pre = torch.stack([F.conv2d(x[g].permute(0, 3, 1, 2), w[g], b[g] if p.bias else None, padding=1) for g in range(G)])
        out.append(dict(x=_padded(x.reshape(G, -1), x_gs), w=_padded(w.permute(0, 1, 3, 4, 2).reshape(G, -1), w_gs),
                        b=_padded(b, b_gs) if p.bias else None, pre=pre, x64=x, w64=w, b64=b))
    return out


def thin_bound(case):
    """max over problems and channels of sum |w| max|x| + |b|: what no partial sum, in any order, exceeds"""
    return max(float((b['w64'].abs().sum((2, 3, 4)) * 4.0 + b['b64'].abs()).max()) for b in thin_build(case))


def thin_pre(case, pi, mut=None):
    b, p = thin_build(case)[pi], case.probs[pi]
    if mut is None:
        return b['pre']
    if mut == 'pad_row':                               # the padding row above the map admitted: the clamped pixel, unscaled
        outs = []
        for g in range(p.groups):
            xp = F.pad(b['x64'][g].permute(0, 3, 1, 2), (1, 1, 1, 1))
            xp[:, :, 0, :] = xp[:, :, 1, :]
            outs.append(F.conv2d(xp, b['w64'][g], b['b64'][g] if p.bias else None))
        return torch.stack(outs)
    assert mut == 'row_lane'                           # the row form keeps lane ow + 1: every pixel holds its right neighbour's
    pre = torch.roll(b['pre'], -1, 4).clone()
    pre[..., -1] = float('nan')
    return pre


def thin_act64(pre, act):
    if act == ACT_RELU:
        return pre.clamp_min(0.0)
    if act == ACT_EXP:
        return pre.exp()
    if act == ACT_CONF:
        return pre.clamp(0.0, 4.0).exp()
    return pre


def thin_exp_args(case, pi):
    """the arguments expf sees in problem pi"""
    p = case.probs[pi]
    pre = thin_pre(case, pi)
    return pre.clamp(0.0, 4.0) if p.act == ACT_CONF else pre


def exp_cpu_err(args):
    """torch-CPU float32 exp against float64 exp: max relative error"""
    a = args.reshape(-1).double()
    return float(((a.float().exp().double() - a.exp()).abs() / a.exp()).max()) if a.numel() else 0.0


THIN_REFUSALS = ['d0', 'n0', 'n5', 'x0', 'w0', 'y0', 'res', 'KH', 'KW', 'stride', 'pad_h', 'pad_w', 'dil_h', 'dil_w', 'y_nchw',
                 'ksplit', 'y_coff', 'act_split', 'N2', 'H2', 'W2', 'Cin2', 'OH', 'OW', 'Cout0', 'Cout5', 'Cin6', 'N0', 'x+4', 'w+4',
                 'x_gs2', 'w_gs2']


# ============================================================================================================================= crop
CROP_S = [15, 16, 127, 255]
CROP_IMAGES = {'frame': (60, 80), 'wide': (240, 320), 'tiny': (8, 5)}      # H, W; 'tiny' is smaller than most windows
CROP_FILL = (13, 200, 77)
CROP_MUTATIONS = ['double_coord']

Crop = collections.namedtuple('Crop', 'image x0 y0 win')


@functools.lru_cache(maxsize=None)
def crop_image(name):
    H, W = CROP_IMAGES[name]
    return _rng('crop', name).integers(0, 256, (H, W, 3)).astype(np.uint8)


def crop_wins(S):
    if S < 100:
        return list(range(1, 2 * S + 4))
    return sorted(set([1, 2, 3] + list(range(S - 2, S + 3)) + list(range(2 * S - 2, 2 * S + 3)) + list(range(37, 1101, 37))))


def crop_origins(H, W, win):
    """(x0, y0): over each border, over each corner, wholly outside on each side"""
    cx, cy, h = (W - win) // 2, (H - win) // 2, win // 2 + 1
    return [(-h, cy), (W - win + h, cy), (cx, -h), (cx, H - win + h), (-h, -h), (W - win + h, -h), (-h, H - win + h),
            (W - win + h, H - win + h), (-win - 3, cy), (W + 2, cy), (cx, -win - 3), (cx, H + 2)]


@functools.lru_cache(maxsize=None)
def crop_cases(S):
    name = 'frame' if S < 100 else 'wide'
    H, W = CROP_IMAGES[name]
    out = [Crop(name, (W - win) // 2, (H - win) // 2, win) for win in crop_wins(S)]
    for win in (S, 2 * S, S + 3, 5):
        out += [Crop(name, x0, y0, win) for x0, y0 in crop_origins(H, W, win)]
    th, tw = CROP_IMAGES['tiny']
    out += [Crop('tiny', (tw - win) // 2, (th - win) // 2, win) for win in (S, 2 * S, S + 3, 7, 3)]
    out += [Crop('tiny', -2, 1, S + 1), Crop('tiny', 3, -4, 2 * S - 1)]
    return out


def crop_pos(case):
    """a target position whose window (track_utils.py:41-44: round(pos - (win + 1) / 2)) starts at the case's origin"""
    return [case.x0 + (case.win + 1) / 2 + 0.25, case.y0 + (case.win + 1) / 2 + 0.25]


def _axis_double(n_src, n_dst):
    """hostutils._resize_axis with the coordinate kept in double up to the floor: what a kernel that skips the float rounding does"""
    scale = 1.0 / (float(n_dst) / float(n_src))
    f = (np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5
    s = np.floor(f).astype(np.int64)
    f = (f - s).astype(np.float32)
    lo = s < 0
    f[lo], s[lo] = 0.0, 0
    hi = s >= n_src - 1
    f[hi], s[hi] = 0.0, n_src - 1
    w1 = np.rint(f * np.float32(2048.0)).astype(np.int64)
    w0 = np.rint((np.float32(1.0) - f) * np.float32(2048.0)).astype(np.int64)
    return s, np.minimum(s + 1, n_src - 1), w0, w1


def resize_with(img, S, axis):
    """hostutils.resize_bilinear_u8's two passes with the axis rule handed in"""
    h, w, _ = img.shape
    if (h, w) == (S, S):
        return img.copy()
    if w == 2 * S and h == 2 * S:
        q = img.astype(np.int64)
        return ((q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    x0, x1, ax0, ax1 = axis(w, S)
    y0, y1, ay0, ay1 = axis(h, S)
    src = img.astype(np.int64)
    rows = src[:, x0, :] * ax0[None, :, None] + src[:, x1, :] * ax1[None, :, None]
    a, b = rows[y0], rows[y1]
    out = (((ay0[:, None, None] * (a >> 4)) >> 16) + ((ay1[:, None, None] * (b >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def crop_ref(case, S, mut=None):
    """-> float32 [3, S, S]: hostutils.get_subwindow_tracking (mean-colour padding, the restated OpenCV resize)"""
    from usot_amd import hostutils
    im = crop_image(case.image)
    if mut is None:
        patch, _ = hostutils.get_subwindow_tracking(im, crop_pos(case), S, case.win, CROP_FILL, out_mode='np')
    else:
        raw, _ = hostutils.get_subwindow_tracking(im, crop_pos(case), case.win, case.win, CROP_FILL, out_mode='np')
        patch = resize_with(raw, S, _axis_double)
    return np.ascontiguousarray(patch.transpose(2, 0, 1)).astype(np.float32)


CROP_SKIPPED = ['im0', 'H0', 'W-1', 'win0']            # batch slots that must stay untouched
CROP_REFUSALS = {'single': ['im0', 'out0', 'H0', 'W0', 'win0', 'S0'], 'batch': ['ctl0', 'out0', 'B0', 'B65536', 'S0', 'S4097']}


# =========================================================================================================================== reduce
CONFS = {1: (1,), 2: (1, 1), 4: (1, 1, 2, 4), 7: (1, 1, 2, 4, 8, 8, 8)}           # sums 1, 2, 8, 32
RED_M, RED_C = [1, 2, 4, 7], [4, 8, 36, 256]
RED_BIG = (4, 1, 65537, 32)                            # B, M, P, C: 2 097 184 channel quads on a grid capped at 8192 x 256
RED_CAP = 8192 * 256
RED_MUTATIONS = ['map_weighted', 'map_distinct']
# (map, confidences of the MAPS): the sum over the SLOTS is a power of two; maps no slot names carry 8
RED_MAPS = [((0, 1), CONFS[2]), ((1, 0), CONFS[2]), ((1, 1), (8, 1)),
            ((0, 1, 2, 3), CONFS[4]), ((3, 2, 1, 0), CONFS[4]), ((2, 2, 2, 2), (8, 8, 2, 8)),
            ((0, 1, 2, 3, 4, 5, 6), CONFS[7]), ((6, 5, 4, 3, 2, 1, 0), CONFS[7]), ((0, 1, 2, 3, 3, 3, 3), (1, 1, 2, 1, 8, 8, 8))]
RED_DTYPES = [(i, o) for i in (0, 1, 2) for o in (1, 2)]                          # usot_conf_fusion_reduce_lp's in_dtype, out_dtype
LP_TORCH = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}

Red = collections.namedtuple('Red', 'B M P C')


def reduce_cases():
    return [Red(2, m, 5, c) for m in RED_M for c in RED_C]


def reduce_operands(case, map_confs=None):
    """cv [B * M, P, 2 C] float32: confidences in channels [0, C), values in [C, 2 C)"""
    B, M, P, C = case
    g = _rng('reduce', tuple(case), map_confs)
    scale = 2.0 ** g.integers(-3, 4, (B, 1, P, C))
    if map_confs is None:
        rot = g.integers(0, M, (B, 1, P, C))
        conf = np.asarray(CONFS[M], np.float64)[(np.arange(M).reshape(1, M, 1, 1) + rot) % M] * scale
    else:
        conf = np.asarray(map_confs, np.float64).reshape(1, M, 1, 1) * scale
    val = g.integers(-255, 256, (B, M, P, C)) / 4
    return torch.from_numpy(np.concatenate([conf, val], 3).reshape(B * M, P, 2 * C)).float()


def reduce_ref(cv, case, slot_map=None, mut=None):
    """connect.py:132-142 in float64 with the reference's association: normalise each confidence, weight, add in slot order
    -> out [B, P, C], den [B, P, C]"""
    B, M, P, C = case
    cv = cv.double().reshape(B, M, P, 2 * C)
    slots = list(slot_map) if slot_map is not None else list(range(M))
    weight = [1.0] * len(slots)
    if mut == 'map_weighted':                          # each slot's confidence scaled by how many slots name its map
        weight = [float(slots.count(s)) for s in slots]
    elif mut == 'map_distinct':                        # one term per distinct map
        slots = sorted(set(slots), key=slots.index)
        weight = [1.0] * len(slots)
    den = sum(k * cv[:, s, :, :C] for s, k in zip(slots, weight))
    out = sum((k * cv[:, s, :, :C] / den) * cv[:, s, :, C:] for s, k in zip(slots, weight))
    return out, den


def stored(ref, dtype):
    """the float64 reference as a correct kernel stores it (exact in fp32; one round-to-nearest-even to a 16-bit type)"""
    return ref.float().to(dtype)


RED_REFUSALS = {'f32': ['cv0', 'out0', 'B0', 'M0', 'P0', 'C0', 'C6', 'cv+4', 'out+4'],
                'lp': ['cv0', 'out0', 'B0', 'M0', 'P0', 'C0', 'C6', 'cv+4', 'out+4', 'out_dtype0', 'out_dtype3', 'in_dtype-1', 'in_dtype3'],
                'map': ['cv0', 'out0', 'B0', 'M0', 'P0', 'C0', 'C6', 'cv+4', 'out+4', 'map+2']}


# =========================================================================================================================== movers
PERMS = list(itertools.permutations(range(4)))
PERM_SHAPES = [(3, 4, 5, 6), (3, 1, 5, 6)]
PERM_BIG = (123377, 1, 17, 1)                          # 2 097 152 + 256 + 1 elements: one past a second full pass of 8192 x 256
PERM_CAP = 8192 * 256
ROWS_BIG = (2050, 1024, 2100)                          # rows moved, row length, rows of the bank: 524 800 quads > 2048 x 256
ROWS_CAP = 2048 * 256
MULTI_BIG = (1030, [1024, 64, 256, 12], 1100)          # rows moved, row lengths, rows of each bank: 263 680 quads > 1024 x 256
MULTI_CAP = 1024 * 256


def perm_source(shape, sliced):
    """-> (base tensor, the 4-D source view): dense, or a strided slice of a larger tensor"""
    if not sliced:
        base = torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(shape) / 4
        return base, base
    big = tuple(2 * s + 3 for s in shape)
    base = torch.arange(int(np.prod(big)), dtype=torch.float32).reshape(big) / 4
    return base, base[1:1 + shape[0], 2:2 + 2 * shape[1]:2, 0:shape[2], 3:3 + shape[3]]


def gather_rows(n, bank_rows, key):
    """row indices with repeats"""
    return _rng('gather', n, bank_rows, key).integers(0, bank_rows, n).astype(np.int32)


def scatter_rows(n, bank_rows, key):
    """distinct row indices"""
    return _rng('scatter', n, bank_rows, key).permutation(bank_rows)[:n].astype(np.int32)


def rows_data(rows, length, key):
    return torch.from_numpy(_rng('rows', rows, length, key).integers(-2 ** 20, 2 ** 20, (rows, length)) / 4).float()


# ============================================================================================================ batch append + gather
AG_MUTATIONS = ['app_first']
AG = dict(B=6, cap=4, n_pick=7, lens=[8, 12, 4, 16])
AG['bank_rows'] = AG['B'] * AG['cap']
AG['append'] = [2, -1, AG['bank_rows'], INT32_MIN, INT32_MAX, 21]
AG['picks'] = [[0, 2, 1, 2, 3, 23, 5],                                                # in range; the appended row twice
               [-1, 4, -1, 5, 6, 7, 0],                                               # pick == append_row == -1: zeros
               [AG['bank_rows'], 8, AG['bank_rows'] + 1, 9, AG['bank_rows'], 10, 11],
               [INT32_MIN, INT32_MAX, 12, INT32_MIN, 13, -1, 14],
               [INT32_MAX, INT32_MIN, 16, INT32_MAX, AG['bank_rows'], 17, 18],
               [21, -1, AG['bank_rows'], INT32_MIN, INT32_MAX, 20, 21]]                # every kind beside in-range picks


def ag_ref(fresh, banks, mut=None):
    """include/usot_hip.h: slot b's fresh row -> bank row append_row, picks[j] -> picked row b * n_pick + j, a pick equal to
    append_row read from the fresh row; a row outside [0, bank_rows) is never touched: such an append is dropped, such a pick
    gathers zeros.  fresh[k] [B, len], banks[k] [bank_rows, len] -> (banks after, picked[0..2])"""
    B, nq, rows = AG['B'], AG['n_pick'], AG['bank_rows']
    after = [b.clone() for b in banks]
    picked = [torch.zeros(B * nq, n) for n in AG['lens'][1:]]
    for b in range(B):
        app = AG['append'][b]
        if 0 <= app < rows:
            for k in range(4):
                after[k][app] = fresh[k][b]
        for j, r in enumerate(AG['picks'][b]):
            for k in range(1, 4):
                if mut == 'app_first' and r == app:
                    picked[k - 1][b * nq + j] = fresh[k][b]
                elif 0 <= r < rows:
                    picked[k - 1][b * nq + j] = fresh[k][b] if r == app else banks[k][r]
    return after, picked
