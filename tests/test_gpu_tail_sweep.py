"""GPU: the kernels that open and close a frame (csrc/head_ops.hip, head_common.h, multitrack.hip) against the references of
tests/tail_cases.py:

  decode   usot_decode_f32 at S 1 .. 64, usot_decode_dev_f32 at S 2 .. 64, usot_decode_batch_f32 at S 2 .. 32 with 1 and 5 slots: a
           planted winner in every placement class (cell 0, the last cell, both sides of the first wavefront boundary, cells 1023
           and 1024), exact ties inside a wave, across waves, inside one thread's passes and with the later cell on a lower thread,
           NaNs in either map and in the box, the all-NaN maps, boxes that fire all four RoI clamps;
  thin     usot_thin_conv3x3_f32 per pixel at six Cin, every Cout, five shapes, four activations, 1 .. 4 problems, groups with padded
           strides, null biases; per row at W 1, 2, 25, 63, 64 with every Cout and every way the launcher splits (or keeps) a
           4-channel problem, bit-equal to the per-pixel form; W = 65 and 1023 rows, which stay per pixel;
  crop     usot_crop_resize_u8_f32 and its batch at S 15, 16, 127, 255: every window edge of the two small sizes, the edges around S
           and 2 S and every 37th up to 1073 of the two large, windows over each border and corner, wholly outside, an 8 x 5 image;
  reduce   usot_conf_fusion_reduce_f32 / _lp / _map_f32 at M 1, 2, 4, 7, C 4 .. 256, six type pairs, nine slot maps, one map past the
           grid cap;
  movers   usot_permute4_f32 in all 24 axis orders (dense and sliced sources, a dim of 1, one tensor past the grid cap),
           usot_rows_copy_f32 and usot_rows_copy_multi_f32 past their caps, every untouched row checked;
  gather   usot_rows_append_gather_batch_f32 with picks and append rows at -1, bank_rows, INT32_MIN and INT32_MAX;
  everything the launchers refuse: USOT_EINVAL and the output's bits untouched.

Every comparison is an EQUALITY of bits (a NaN equals a NaN; under the two exact thin-conv activations +0 equals -0), except the
decode's score (1e-6), penalty and pscore (rtol 1e-9) and the thin heads' expf (tail_cases.EXP_ALLOW).  Outputs are NaN-prefilled
between canaries (tests/guarded.py), inputs lie between NaNs, every test ends with guarded.check.  One item loops over its list and
reports every failing case.  The lists are asserted by tests/test_tail_lists.py."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded  # noqa: E402
import tail_cases as tc  # noqa: E402
from usot_amd import hip  # noqa: E402
from usot_amd.engine import SLOT_REC, STEP_HDR  # noqa: E402

DEV = 'cuda:0'
EINVAL = -1
CANARY64 = np.array([0x7FC17FC17FC17FC1], np.uint64).view(np.int64)[0]
CANARY32 = np.array([tc.CANARY32], np.uint32).view(np.int32)[0]


def L():
    return hip.lib()


def st():
    return hip.stream()


def P(t, offset=0):
    """the address of a device tensor (+ bytes), None for None"""
    return None if t is None else C.c_void_p(t.data_ptr() + offset)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32, 2: np.int16, 1: np.uint8}[a.dtype.itemsize])


def host(t):
    """device tensor -> numpy (16-bit floats as their int16 words)"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy() if t.dtype in (torch.float16, torch.bfloat16) else t.numpy()


def differ(got, want, nan_ok=False):
    """'' when `got` holds the bits of `want` (with nan_ok: a NaN equals a NaN), else what differs"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return 'shape %s, want %s' % (got.shape, want.shape)
    ne = bits(got) != bits(want)
    if nan_ok:
        ne &= ~(np.isnan(got) & np.isnan(want))
    if not ne.any():
        return ''
    first = tuple(int(i) for i in np.argwhere(ne)[0])
    return '%d of %d elements differ, first at %s: got %r, want %r' % (int(ne.sum()), ne.size, first, got[first], want[first])


def untouched(a):
    """every word of a (numpy view of a) canary-prefilled buffer still holds the canary"""
    b = bits(a)
    return bool((b == {8: CANARY64, 4: CANARY32}[b.dtype.itemsize]).all())


def finish(what, start, launches, bad):
    torch.cuda.synchronize()
    guarded.check(start)
    print('%s: %d cases, %d failing' % (what, launches, len(bad)))
    assert not bad, bad[:20]


def ctl_block(B, tag):
    ctl = np.zeros(STEP_HDR + B * SLOT_REC.itemsize, np.uint8)
    ctl[:8].view(np.float64)[0] = tag
    return ctl, ctl[STEP_HDR:].view(SLOT_REC)


# =========================================================================================================================== decode
def close(got, want, atol=0.0, rtol=0.0):
    return (np.isnan(got) and np.isnan(want)) or abs(got - want) <= atol + rtol * abs(want)


def decode_check(o, ref, written, roi=None, slot=0.0):
    """one result row against the float64 restatement -> failure texts.  `written`: how many doubles the kernel stores"""
    bad = []
    if not o[0] == ref['i']:
        return ['index %r, want %d' % (o[0], ref['i'])]
    m = differ(o[3:7], ref['box'], nan_ok=True)
    bad += ['box: ' + m] if m else []
    bad += ['score %r, want %r' % (o[1], ref['sc'])] if not close(o[1], float(ref['sc']), atol=1e-6) else []
    bad += ['penalty %r, want %r' % (o[2], ref['pen'])] if not close(o[2], ref['pen'], rtol=1e-9) else []
    bad += ['pscore %r, want %r' % (o[7], ref['ps'])] if not close(o[7], ref['ps'], rtol=1e-9) else []
    bad += ['doubles behind the results were written'] if not untouched(o[written:]) else []
    if roi is not None:
        m = differ(roi[1:], ref['roi'], nan_ok=True)
        bad += ['roi: ' + m] if m else []
        bad += ['roi[0] %r' % roi[0]] if roi[0] != slot else []
    return bad


def decode_inputs(cases):
    """guarded device copies of the stacked operands of a list of cases of one S -> cls [K, n], cls_mem, bbox [K, 4, n], window,
    [(tw, th)]"""
    ops = [tc.decode_operands(c) for c in cases]
    put = lambda k: guarded.put(torch.from_numpy(np.stack([o[k] for o in ops])), DEV)
    return put(0), put(1), put(2), guarded.put(torch.from_numpy(tc.window(cases[0].S)), DEV), [(o[3], o[4]) for o in ops]


def decode_dev(cases, cls, cm, bbox, win, tsz, tag0=1000.0):
    """usot_decode_dev_f32 on every case -> return codes, out [K, 16], roi [K, 5] (numpy)"""
    S, K = cases[0].S, len(cases)
    ctl = np.zeros((K, 8))
    for k, (tw, th) in enumerate(tsz):
        ctl[k, 0], ctl[k, 1], ctl[k, 6] = tw, th, tag0 + k
    ctl = guarded.put(torch.from_numpy(ctl), DEV)
    out = guarded.alloc((K, 16), torch.float64, DEV)
    roi = guarded.alloc((K, 5), torch.float32, DEV)
    rcs = [L().usot_decode_dev_f32(st(), P(cls[k]), P(cm[k]), P(bbox[k]), P(win), P(out[k]), S, tc.instance_size(S), tc.STRIDE, tc.RATIO,
                                   tc.PENALTY_K, c.wi, P(ctl[k]), P(roi[k])) for k, c in enumerate(cases)]
    return rcs, host(out), host(roi)


S_CHUNKS = [(1, 17), (17, 33), (33, 45), (45, 56), (56, 65)]


@pytest.mark.parametrize('lo,hi', S_CHUNKS)
def test_decode_f32(lo, hi):
    """usot_decode_f32: index equal, box bit-equal, score / penalty / pscore within the decode's bars, nothing behind out[7] written."""
    start = guarded.registry_size()
    bad, count = [], 0
    for S in range(lo, hi):
        cases = tc.decode_cases(S)
        cls, cm, bbox, win, tsz = decode_inputs(cases)
        out = guarded.alloc((len(cases), 16), torch.float64, DEV)
        rcs = [L().usot_decode_f32(st(), P(cls[k]), P(cm[k]), P(bbox[k]), P(win), P(out[k]), S, tc.instance_size(S), tc.STRIDE, tc.RATIO,
                                   tc.PENALTY_K, c.wi, tsz[k][0], tsz[k][1]) for k, c in enumerate(cases)]
        o = host(out)
        for k, c in enumerate(cases):
            bad += [(tuple(c), m) for m in (['return code %d' % rcs[k]] if rcs[k] else decode_check(o[k], tc.decode_expected(c), 8))]
        count += len(cases)
    finish('decode S %d .. %d' % (lo, hi - 1), start, count, bad)


@pytest.mark.parametrize('lo,hi', [(max(lo, 2), hi) for lo, hi in S_CHUNKS])
def test_decode_dev(lo, hi):
    """usot_decode_dev_f32: the same, the target size from device memory, the tag behind the results, the RoI (clamped one grid gap
    outside the axis, a NaN kept) bit-equal to the float64 restatement stored as float32."""
    start = guarded.registry_size()
    bad, count = [], 0
    for S in range(lo, hi):
        cases = tc.decode_cases(S)
        rcs, o, r = decode_dev(cases, *decode_inputs(cases))
        for k, c in enumerate(cases):
            if rcs[k]:
                bad.append((tuple(c), 'return code %d' % rcs[k]))
                continue
            bad += [(tuple(c), m) for m in decode_check(o[k], tc.decode_expected(c), 9, r[k])]
            bad += [(tuple(c), 'tag %r' % o[k, 8])] if o[k, 8] != 1000.0 + k else []
        count += len(cases)
    finish('decode_dev S %d .. %d' % (lo, hi - 1), start, count, bad)


@pytest.mark.parametrize('B', tc.DEC_BATCH_B)
def test_decode_batch(B):
    """usot_decode_batch_f32 at S 2 .. 32: every slot bit-equal to usot_decode_dev_f32 on that slot (and so to the reference, which
    test_decode_dev holds it to), the slot index in roi[0], the step tag behind the results.  B = 5: every case at the project's
    window_influence, five consecutive ones per launch; B = 1: every ninth."""
    start = guarded.registry_size()
    bad, count = [], 0
    for S in tc.DEC_S_BATCH:
        cases = [c for c in tc.decode_cases(S) if c.wi == tc.WINDOW_INFLUENCE]
        cases = cases[::9] if B == 1 else cases + cases[:-len(cases) % B]
        cls, cm, bbox, win, tsz = decode_inputs(cases)
        rcs, o1, r1 = decode_dev(cases, cls, cm, bbox, win, tsz)
        out = guarded.alloc((len(cases), 16), torch.float64, DEV)
        roi = guarded.alloc((len(cases), 5), torch.float32, DEV)
        for k in range(0, len(cases), B):
            ctl, recs = ctl_block(B, 77.0 + k)
            recs['tsz'] = tsz[k:k + B]
            rc = L().usot_decode_batch_f32(st(), P(cls[k]), P(cm[k]), P(bbox[k]), P(win), P(out[k]), B, S, tc.instance_size(S), tc.STRIDE,
                                           tc.RATIO, tc.PENALTY_K, tc.WINDOW_INFLUENCE, P(guarded.put(torch.from_numpy(ctl), DEV)),
                                           P(roi[k]))
            bad += [((S, k), 'return code %d' % rc)] if rc or any(rcs[k:k + B]) else []
        o, r = host(out), host(roi)
        for k, c in enumerate(cases):
            m = differ(o[k, :8], o1[k, :8], nan_ok=True) or differ(r[k, 1:], r1[k, 1:], nan_ok=True)
            bad += [(tuple(c), 'differs from decode_dev: ' + m)] if m else []
            bad += [(tuple(c), 'slot %r tag %r' % (r[k, 0], o[k, 8]))] if r[k, 0] != k % B or o[k, 8] != 77.0 + k - k % B else []
            bad += [(tuple(c), 'doubles behind the tag were written')] if not untouched(o[k, 9:]) else []
        count += len(cases)
    finish('decode_batch B %d' % B, start, count, bad)


@pytest.mark.parametrize('entry', ['f32', 'dev', 'batch'])
def test_decode_refusals(entry):
    """S 0 and 65 (33 for the batch), B 0 and 65536, each null pointer: USOT_EINVAL, out and roi untouched; the launch itself is fine."""
    start = guarded.registry_size()
    case = tc.Dec(25, 'win', (63,), tc.WINDOW_INFLUENCE)
    cls, cm, bbox, win, tsz = decode_inputs([case])
    ctl8 = guarded.put(torch.tensor([tsz[0][0], tsz[0][1], 0, 0, 0, 0, 5.0, 0], dtype=torch.float64), DEV)
    blk, recs = ctl_block(1, 5.0)
    recs['tsz'] = tsz
    blk = guarded.put(torch.from_numpy(blk), DEV)
    bad = []
    for rid in ['ok'] + tc.DEC_REFUSALS[entry]:
        out = guarded.alloc((16,), torch.float64, DEV)
        roi = guarded.alloc((5,), torch.float32, DEV)
        a = dict(cls=cls, cls_mem=cm, bbox=bbox, window=win, out=out, tsz=ctl8, ctl=blk, roi=roi, S=25, B=1)
        if rid[0] in 'SB' and rid != 'ok':
            a[rid[0]] = int(rid[1:])
        elif rid != 'ok':
            a[rid[:-1]] = None
        head = (st(), P(a['cls']), P(a['cls_mem']), P(a['bbox']), P(a['window']), P(a['out']))
        tail = (tc.instance_size(25), tc.STRIDE, tc.RATIO, tc.PENALTY_K, tc.WINDOW_INFLUENCE)
        if entry == 'f32':
            rc = L().usot_decode_f32(*head, a['S'], *tail, *tsz[0])
        elif entry == 'dev':
            rc = L().usot_decode_dev_f32(*head, a['S'], *tail, P(a['tsz']), P(a['roi']))
        else:
            rc = L().usot_decode_batch_f32(*head, a['B'], a['S'], *tail, P(a['ctl']), P(a['roi']))
        torch.cuda.synchronize()
        o, r = host(out), host(roi)
        if rid == 'ok':
            bad += [(rid, m) for m in (['return code %d' % rc] if rc else decode_check(o, tc.decode_expected(case), 8 if entry == 'f32' else 9,
                                                                                         None if entry == 'f32' else r))]
        elif rc != EINVAL or not untouched(o) or not untouched(r):
            bad.append((rid, 'return code %d' % rc, 'untouched' if untouched(o) and untouched(r) else 'THE OUTPUT WAS WRITTEN'))
    finish('decode refusals (%s)' % entry, start, len(tc.DEC_REFUSALS[entry]), bad)


# ============================================================================================================================= thin
def thin_put(case):
    """guarded device copies of a case's operands -> per problem (x, w, b)"""
    out, shared = [], None
    for b in tc.thin_build(case):
        if case.share:
            shared = shared if shared is not None else guarded.put(b['x'], DEV)
        out.append((shared if case.share else guarded.put(b['x'], DEV), guarded.put(b['w'], DEV),
                    guarded.put(b['b'], DEV) if b['b'] is not None else None))
    return out


def thin_descs(case, dev, ys, tile=0):
    arr = (hip.ConvDesc * 4)()
    for pi, (p, (x, w, b), y) in enumerate(zip(case.probs, dev, ys)):
        x_gs, w_gs, b_gs, y_gs = tc.thin_strides(case, pi)
        arr[pi] = hip.conv_desc(x.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None, y.data_ptr(), N=case.N, H=case.H,
                                W=case.W, Cin=case.Cin, OH=case.H, OW=case.W, Cout=p.cout, KH=3, KW=3, pad=(1, 1), act=p.act, y_nchw=1,
                                groups=p.groups, x_gs=x_gs, w_gs=w_gs, b_gs=b_gs, y_gs=y_gs, tile=tile)
    return arr


def thin_outs(case):
    return [guarded.alloc((p.groups * tc.thin_strides(case, pi)[3],), torch.float32, DEV) for pi, p in enumerate(case.probs)]


def thin_run(case, dev, tile=0):
    ys = thin_outs(case)
    return L().usot_thin_conv3x3_f32(st(), thin_descs(case, dev, ys, tile), len(case.probs)), ys


def thin_check(case, ys, worst):
    """every problem's output against float64 -> failure texts; worst[0] collects the largest expf error"""
    bad = []
    for pi, (p, y) in enumerate(zip(case.probs, ys)):
        y_gs = tc.thin_strides(case, pi)[3]
        n = case.N * p.cout * case.H * case.W
        got = host(y).reshape(p.groups, y_gs)
        bad += ['problem %d: the gap between groups was written' % pi] if not untouched(got[:, n:]) else []
        got = got[:, :n].reshape(p.groups, case.N, p.cout, case.H, case.W)
        want = tc.thin_act64(tc.thin_pre(case, pi), p.act)
        if p.act in tc.EXACT_ACTS:
            m = differ(got + np.float32(0), want.float().numpy() + np.float32(0))
            bad += ['problem %d: %s' % (pi, m)] if m else []
        else:
            err = np.abs(got.astype(np.float64) - want.numpy()) / want.numpy()
            err = float(np.nan_to_num(err, nan=np.inf).max())
            worst[0] = max(worst[0], err)
            bad += ['problem %d: expf off by %.3e relative (allowed %.3e)' % (pi, err, tc.EXP_ALLOW)] if not err <= tc.EXP_ALLOW else []
    return bad


@pytest.mark.parametrize('which', ['cin%d' % c for c in tc.THIN_CIN] + ['multi'])
def test_thin_per_pixel(which):
    """The wavefront-per-pixel form: lanes that skip the channel loop (Cin 4, 64, 252), run it once (256) and twice (260, 512), every
    Cout, five shapes from 1 x 1, four activations, 1 .. 4 problems, groups with padded strides, null biases."""
    start = guarded.registry_size()
    cases = tc.thin_multi_cases() if which == 'multi' else tc.thin_pixel_cases(int(which[3:]))
    bad, worst = [], [0.0]
    for case in cases:
        assert tc.thin_plan(case)[0] == 'pixel'
        rc, ys = thin_run(case, thin_put(case))
        bad += [(tuple(case), m) for m in (['return code %d' % rc] if rc else thin_check(case, ys, worst))]
    print('largest expf error %.3e (torch-CPU float32: %.3e, allowed %.3e)' % (worst[0], tc.EXP_CPU_ERR, tc.EXP_ALLOW))
    finish('thin conv per pixel, %s' % which, start, len(cases), bad)


def thin_both_forms(case, worst):
    """the launcher's own choice and the per-pixel form (tile = 70): each against float64, and bit-equal to each other"""
    dev = thin_put(case)
    bad = []
    rc, ys = thin_run(case, dev)
    rc70, ys70 = thin_run(case, dev, 70)
    if rc or rc70:
        return ['return codes %d, %d' % (rc, rc70)]
    bad += thin_check(case, ys, worst) + ['tile 70: ' + m for m in thin_check(case, ys70, worst)]
    bad += ['problem %d: the two forms differ: %s' % (pi, m) for pi, (a, b) in enumerate(zip(ys, ys70)) for m in [differ(host(a), host(b), True)]
            if m]
    return bad


@pytest.mark.parametrize('W', tc.ROW_W)
def test_thin_per_row(W):
    """The wavefront-per-row form (Cin 256, 1032 rows) at W 1, 2, 25, 63, 64 and every Cout; with Cout 4 the first of the three
    problems runs as two of 2 channels."""
    start = guarded.registry_size()
    bad, worst = [], [0.0]
    for case in tc.thin_row_cases(W):
        assert tc.thin_plan(case)[0] == 'row'
        bad += [(tuple(case), m) for m in thin_both_forms(case, worst)]
    print('largest expf error %.3e (allowed %.3e)' % (worst[0], tc.EXP_ALLOW))
    finish('thin conv per row, W %d' % W, start, 4, bad)


@pytest.mark.parametrize('k', range(8), ids=['single4_w2', 'single4_w25', 'two4_of_three', 'one4_of_four', 'four_in_two_groups', 'w65',
                                             'rows1023', 'rows1024'])
def test_thin_splits_and_thresholds(k):
    """Every way the row form treats a 4-channel problem (split alone; only the first of two split; none split beside three others;
    never split in groups), and the thresholds: W = 65 and 1023 rows stay per pixel, 1024 rows go per row."""
    case, form, split, why = tc.thin_split_cases()[k]
    assert tc.thin_plan(case) == (form, split), why
    start = guarded.registry_size()
    worst = [0.0]
    bad = thin_both_forms(case, worst)
    finish('thin conv: %s' % why, start, 1, bad)


def test_thin_refusals():
    """One launch per clause of the launcher's if chain: USOT_EINVAL and no output written; the unchanged launch is right."""
    start = guarded.registry_size()
    case = tc.Thin(2, 3, 4, 8, (tc.P(2), tc.P(1, tc.ACT_RELU)), False)
    dev = thin_put(case)
    bad = []
    for rid in ['ok'] + tc.THIN_REFUSALS:
        ys = thin_outs(case)
        d = thin_descs(case, dev, ys)
        n, arr = 2, d
        if rid == 'd0':
            arr = None
        elif rid in ('n0', 'n5'):
            n = int(rid[1])
        elif rid in ('x0', 'w0', 'y0'):
            setattr(d[1], rid[0], None)
        elif rid == 'res':
            d[1].res = dev[1][0].data_ptr()
        elif rid in ('KH', 'KW'):
            setattr(d[1], rid, 1)
        elif rid in ('stride', 'dil_h', 'dil_w', 'ksplit'):
            setattr(d[1], rid, 2)
        elif rid in ('pad_h', 'pad_w', 'y_nchw'):
            setattr(d[1], rid, 0)
        elif rid in ('y_coff', 'act_split'):
            setattr(d[1], rid, 1)
        elif rid == 'N2':
            d[1].N += 1
        elif rid == 'H2':
            d[1].H = d[1].OH = case.H + 1
        elif rid == 'W2':
            d[1].W = d[1].OW = case.W + 1
        elif rid == 'Cin2':
            d[1].Cin += 4
        elif rid in ('OH', 'OW'):
            setattr(d[1], rid, getattr(d[1], rid) + 1)
        elif rid in ('Cout0', 'Cout5'):
            d[1].Cout = int(rid[4])
        elif rid == 'Cin6':
            d[0].Cin = d[1].Cin = 6
        elif rid == 'N0':
            d[0].N = d[1].N = 0
        elif rid in ('x+4', 'w+4'):
            setattr(d[1], rid[0], getattr(d[1], rid[0]) + 4)
        elif rid in ('x_gs2', 'w_gs2'):
            setattr(d[1], rid[:4], 2)
        else:
            assert rid == 'ok', rid
        rc = L().usot_thin_conv3x3_f32(st(), arr, n)
        torch.cuda.synchronize()
        if rid == 'ok':
            bad += [(rid, m) for m in (['return code %d' % rc] if rc else thin_check(case, ys, [0.0]))]
        elif rc != EINVAL or not all(untouched(host(y)) for y in ys):
            bad.append((rid, 'return code %d' % rc, 'untouched' if all(untouched(host(y)) for y in ys) else 'THE OUTPUT WAS WRITTEN'))
    finish('thin conv refusals', start, len(tc.THIN_REFUSALS), bad)


# ============================================================================================================================= crop
@pytest.mark.parametrize('S', tc.CROP_S)
def test_crop_single_and_batch(S):
    """usot_crop_resize_u8_f32 window by window and usot_crop_resize_batch_u8_f32 on the same records in ONE launch: bit-equal to the
    host's crop and to each other; the batch's slots with no image, no rows, no columns or no window keep their bits."""
    start = guarded.registry_size()
    cases = tc.crop_cases(S)
    K = len(cases)
    ims = {name: guarded.put(torch.from_numpy(tc.crop_image(name)), DEV) for name in tc.CROP_IMAGES}
    want = np.stack([tc.crop_ref(c, S) for c in cases])
    single = guarded.alloc((K, 3, S, S), torch.float32, DEV)
    batch = guarded.alloc((K + len(tc.CROP_SKIPPED), 3, S, S), torch.float32, DEV)
    ctl, recs = ctl_block(K + len(tc.CROP_SKIPPED), 3.0)
    rcs = []
    for k, c in enumerate(cases + cases[:len(tc.CROP_SKIPPED)]):
        H, W = tc.CROP_IMAGES[c.image]
        r = recs[k]
        r['im'], r['H'], r['W'], r['x0'], r['y0'], r['win'], r['fill'] = ims[c.image].data_ptr(), H, W, c.x0, c.y0, c.win, tc.CROP_FILL
        if k < K:
            rcs.append(L().usot_crop_resize_u8_f32(st(), P(ims[c.image]), P(single[k]), H, W, c.x0, c.y0, c.win, S, *tc.CROP_FILL))
    for k, rid in enumerate(tc.CROP_SKIPPED):
        field, value = {'im0': ('im', 0), 'H0': ('H', 0), 'W-1': ('W', -1), 'win0': ('win', 0)}[rid]
        recs[K + k][field] = value
    rcb = L().usot_crop_resize_batch_u8_f32(st(), P(guarded.put(torch.from_numpy(ctl), DEV)), P(batch), K + len(tc.CROP_SKIPPED), S)
    bad = [('batch', 'return code %d' % rcb)] if rcb else []
    s, b = host(single), host(batch)
    for k, c in enumerate(cases):
        bad += [(tuple(c), 'return code %d' % rcs[k])] if rcs[k] else []
        bad += [(tuple(c), 'single: ' + m) for m in [differ(s[k], want[k])] if m]
        bad += [(tuple(c), 'batch: ' + m) for m in [differ(b[k], want[k])] if m]
    bad += [(rid, 'the slot was written') for k, rid in enumerate(tc.CROP_SKIPPED) if not untouched(b[K + k])]
    finish('crop S %d' % S, start, K, bad)


def test_crop_refusals():
    start = guarded.registry_size()
    S, c = 15, tc.crop_cases(15)[20]
    H, W = tc.CROP_IMAGES[c.image]
    im = guarded.put(torch.from_numpy(tc.crop_image(c.image)), DEV)
    want = tc.crop_ref(c, S)
    ctl, recs = ctl_block(1, 3.0)
    r = recs[0]
    r['im'], r['H'], r['W'], r['x0'], r['y0'], r['win'], r['fill'] = im.data_ptr(), H, W, c.x0, c.y0, c.win, tc.CROP_FILL
    ctl = guarded.put(torch.from_numpy(ctl), DEV)
    bad = []
    for entry in ('single', 'batch'):
        for rid in ['ok'] + tc.CROP_REFUSALS[entry]:
            out = guarded.alloc((3, S, S), torch.float32, DEV)
            a = dict(im=im, out=out, ctl=ctl, H=H, W=W, win=c.win, S=S, B=1)
            if rid != 'ok':
                a[rid.rstrip('0123456789')] = None if rid[:-1] in ('im', 'out', 'ctl') else int(rid.lstrip('HWwinSB'))
            if entry == 'single':
                rc = L().usot_crop_resize_u8_f32(st(), P(a['im']), P(a['out']), a['H'], a['W'], c.x0, c.y0, a['win'], a['S'], *tc.CROP_FILL)
            else:
                rc = L().usot_crop_resize_batch_u8_f32(st(), P(a['ctl']), P(a['out']), a['B'], a['S'])
            torch.cuda.synchronize()
            if rid == 'ok':
                bad += [(entry, rid, m) for m in (['return code %d' % rc] if rc else [differ(host(out), want)]) if m]
            elif rc != EINVAL or not untouched(host(out)):
                bad.append((entry, rid, 'return code %d' % rc, 'untouched' if untouched(host(out)) else 'THE OUTPUT WAS WRITTEN'))
    finish('crop refusals', start, 12, bad)


# =========================================================================================================================== reduce
def reduce_call(cv, out, case, in_dtype=0, out_dtype=0, smap=None, entry='f32'):
    B, M, Pn, Cn = case
    if entry == 'lp':
        return L().usot_conf_fusion_reduce_lp(st(), P(cv), in_dtype, P(out), B, M, Pn, Cn, out_dtype)
    if entry == 'map':
        return L().usot_conf_fusion_reduce_map_f32(st(), P(cv), P(out), B, M, Pn, Cn, P(smap))
    return L().usot_conf_fusion_reduce_f32(st(), P(cv), P(out), B, M, Pn, Cn)


def test_reduce_f32():
    """usot_conf_fusion_reduce_f32 at M 1, 2, 4, 7 and C 4, 8, 36, 256: the float64 value bit for bit."""
    start = guarded.registry_size()
    bad = []
    for case in tc.reduce_cases():
        cv = tc.reduce_operands(case)
        out = guarded.alloc((case.B, case.P, case.C), torch.float32, DEV)
        rc = reduce_call(guarded.put(cv, DEV), out, case)
        bad += [(tuple(case), m) for m in (['return code %d' % rc] if rc else [differ(host(out), tc.reduce_ref(cv, case)[0].float().numpy())]) if m]
    finish('reduce fp32', start, 16, bad)


@pytest.mark.parametrize('in_dtype,out_dtype', tc.RED_DTYPES)
def test_reduce_lp(in_dtype, out_dtype):
    """usot_conf_fusion_reduce_lp, all six type pairs: the round-to-nearest-even of the float64 value."""
    start = guarded.registry_size()
    bad = []
    for case in tc.reduce_cases():
        cv = tc.reduce_operands(case)
        out = guarded.alloc((case.B, case.P, case.C), tc.LP_TORCH[out_dtype], DEV)
        rc = reduce_call(guarded.put(cv.to(tc.LP_TORCH[in_dtype]), DEV), out, case, in_dtype, out_dtype, entry='lp')
        want = host(tc.stored(tc.reduce_ref(cv, case)[0], tc.LP_TORCH[out_dtype]))
        bad += [(tuple(case), m) for m in (['return code %d' % rc] if rc else [differ(host(out), want)]) if m]
    finish('reduce lp %d -> %d' % (in_dtype, out_dtype), start, 16, bad)


def test_reduce_map():
    """usot_conf_fusion_reduce_map_f32: identity, reversed, constant and steady-state maps, sums over the SLOTS; a null map is the
    plain reduction."""
    start = guarded.registry_size()
    bad = []
    for smap, confs in tc.RED_MAPS:
        for Cn in (8, 36):
            case = tc.Red(2, len(smap), 5, Cn)
            cv = tc.reduce_operands(case, confs)
            dcv = guarded.put(cv, DEV)
            for m_ in (smap, None) if confs == tc.CONFS[len(smap)] else (smap,):     # without the map the sum is a power of two only there
                out = guarded.alloc((case.B, case.P, case.C), torch.float32, DEV)
                dmap = guarded.put(torch.tensor(m_, dtype=torch.int32), DEV) if m_ else None
                rc = reduce_call(dcv, out, case, smap=dmap, entry='map')
                want = tc.reduce_ref(cv, case, m_)[0].float().numpy()
                bad += [(smap, Cn, m_, m) for m in (['return code %d' % rc] if rc else [differ(host(out), want)]) if m]
    finish('reduce map', start, 30, bad)


def test_reduce_past_the_grid_cap():
    """B 4, P 65537, C 32, M 1: 2 097 184 channel quads on a grid capped at 8192 blocks of 256 - threads 0 .. 31 run their loop twice."""
    start = guarded.registry_size()
    case = tc.Red(*tc.RED_BIG)
    assert case.B * case.P * case.C // 4 > tc.RED_CAP
    cv = tc.reduce_operands(case)
    out = guarded.alloc((case.B, case.P, case.C), torch.float32, DEV)
    rc = reduce_call(guarded.put(cv, DEV), out, case)
    bad = ['return code %d' % rc] if rc else [m for m in [differ(host(out), tc.reduce_ref(cv, case)[0].float().numpy())] if m]
    finish('reduce past the cap', start, 1, bad)


@pytest.mark.parametrize('entry', ['f32', 'lp', 'map'])
def test_reduce_refusals(entry):
    start = guarded.registry_size()
    case = tc.Red(2, 2, 5, 8)
    cv = tc.reduce_operands(case)
    dt = torch.float16 if entry == 'lp' else torch.float32
    dcv = guarded.put(cv.to(dt), DEV)
    dmap = guarded.put(torch.tensor([1, 0, 0, 0], dtype=torch.int32), DEV)
    want = host(tc.stored(tc.reduce_ref(cv, case, (1, 0) if entry == 'map' else None)[0], dt))
    bad = []
    for rid in ['ok'] + tc.RED_REFUSALS[entry]:
        out = guarded.alloc((case.B * case.P * case.C + 8,), dt, DEV)
        a = dict(cv=P(dcv), out=P(out), map=P(dmap), B=case.B, M=case.M, P=case.P, C=case.C, in_dtype=1, out_dtype=1)
        if rid in ('cv0', 'out0'):
            a[rid[:-1]] = None
        elif '+' in rid:
            name, off = rid.split('+')
            a[name] = P({'cv': dcv, 'out': out, 'map': dmap}[name], int(off))
        elif rid != 'ok':
            name = rid.rstrip('-0123456789')
            a[name] = int(rid[len(name):])
        rc = _reduce_raw(entry, a)
        torch.cuda.synchronize()
        o = host(out)
        if rid == 'ok':
            bad += [(rid, m) for m in (['return code %d' % rc] if rc else [differ(o[:-8].reshape(want.shape), want)]) if m]
        elif rc != EINVAL or not _canary16(o, dt):
            bad.append((rid, 'return code %d' % rc, 'untouched' if _canary16(o, dt) else 'THE OUTPUT WAS WRITTEN'))
    finish('reduce refusals (%s)' % entry, start, len(tc.RED_REFUSALS[entry]), bad)


def _reduce_raw(entry, a):
    if entry == 'lp':
        return L().usot_conf_fusion_reduce_lp(st(), a['cv'], a['in_dtype'], a['out'], a['B'], a['M'], a['P'], a['C'], a['out_dtype'])
    if entry == 'map':
        return L().usot_conf_fusion_reduce_map_f32(st(), a['cv'], a['out'], a['B'], a['M'], a['P'], a['C'], a['map'])
    return L().usot_conf_fusion_reduce_f32(st(), a['cv'], a['out'], a['B'], a['M'], a['P'], a['C'])


def _canary16(o, dt):
    return bool((o == np.int16(guarded.CANARY)).all()) if dt == torch.float16 else untouched(o)


# =========================================================================================================================== movers
def permute_case(shape, perm, sliced):
    base, view = tc.perm_source(shape, sliced)
    dbase = guarded.put(base, DEV)
    src = view.permute(perm)
    dst = guarded.alloc(tuple(src.shape), torch.float32, DEV)
    rc = L().usot_permute4_f32(st(), P(dbase, 4 * view.storage_offset()), P(dst), *src.shape, *src.stride())
    return ['return code %d' % rc] if rc else [m for m in [differ(host(dst), src.contiguous().numpy())] if m]


def test_permute4_every_order():
    """usot_permute4_f32: all 24 axis orders of a 3 x 4 x 5 x 6 and a 3 x 1 x 5 x 6 source, dense and as a strided slice of a larger
    tensor."""
    start = guarded.registry_size()
    bad = [(shape, perm, sliced, m) for shape in tc.PERM_SHAPES for perm in tc.PERMS for sliced in (False, True)
           for m in permute_case(shape, perm, sliced)]
    finish('permute4', start, 96, bad)


def test_permute4_past_the_grid_cap():
    """2 097 152 + 256 + 1 elements on a grid capped at 8192 blocks of 256: a second pass of one full block and one thread more."""
    start = guarded.registry_size()
    bad = permute_case(tc.PERM_BIG, (1, 2, 3, 0), False)
    finish('permute4 past the cap', start, 1, bad)


def rows_expected_scatter(src, idx, rows):
    """numpy [rows, len] with the canary in every row the scatter does not name"""
    want = np.full((rows, src.shape[1]), 0, np.int32)
    want[:] = CANARY32
    want[idx] = bits(src.numpy())
    return want.view(np.float32)


def test_rows_copy_past_the_grid_cap():
    """usot_rows_copy_f32: a gather and a scatter of 2050 rows of 1024 floats (524 800 quads, the grid capped at 2048 blocks of 256);
    the 50 rows the scatter does not name keep their bits."""
    start = guarded.registry_size()
    n, length, rows = tc.ROWS_BIG
    bank = tc.rows_data(rows, length, 'bank')
    gi, si = tc.gather_rows(n, rows, 0), tc.scatter_rows(n, rows, 0)
    out = guarded.alloc((n, length), torch.float32, DEV)
    rc = L().usot_rows_copy_f32(st(), P(guarded.put(bank, DEV)), P(guarded.put(torch.from_numpy(gi), DEV)), P(out), n, length, 0)
    bad = ['gather: return code %d' % rc] if rc else ['gather: ' + m for m in [differ(host(out), bank.numpy()[gi])] if m]
    src = tc.rows_data(n, length, 'src')
    dst = guarded.alloc((rows, length), torch.float32, DEV)
    rc = L().usot_rows_copy_f32(st(), P(guarded.put(src, DEV)), P(guarded.put(torch.from_numpy(si), DEV)), P(dst), n, length, 1)
    bad += ['scatter: return code %d' % rc] if rc else ['scatter: ' + m for m in [differ(host(dst), rows_expected_scatter(src, si, rows))] if m]
    finish('rows_copy past the cap', start, 2, bad)


@pytest.mark.parametrize('nseg', [1, 2, 3, 4, 5], ids=['1', '2', '3', '4', '4_long_first'])
def test_rows_copy_multi_past_the_grid_cap(nseg):
    """usot_rows_copy_multi_f32 with 1 .. 4 banks of unequal row length, 1030 rows, the longest (1024 floats: 263 680 quads on a grid
    capped at 1024 blocks of 256) last or first: gather with the three stashed words, and scatter."""
    start = guarded.registry_size()
    n, lens, rows = tc.MULTI_BIG
    lens = lens if nseg == 5 else sorted(lens)[4 - nseg:]
    nseg = len(lens)
    pp = lambda ts: (C.c_void_p * 4)(*([t.data_ptr() for t in ts] + [0] * (4 - len(ts))))
    rl = (C.c_int32 * 4)(*(lens + [0] * (4 - nseg)))
    banks = [tc.rows_data(rows, v, 'multi%d' % k) for k, v in enumerate(lens)]
    gi = np.concatenate([tc.gather_rows(n, rows, nseg), np.array([77, -5, 123456], np.int32)])
    outs = [guarded.alloc((n, v), torch.float32, DEV) for v in lens]
    stash = guarded.alloc((3,), torch.int32, DEV)
    rc = L().usot_rows_copy_multi_f32(st(), nseg, pp([guarded.put(b, DEV) for b in banks]), P(guarded.put(torch.from_numpy(gi), DEV)),
                                      pp(outs), n, rl, 0, P(stash))
    bad = ['gather: return code %d' % rc] if rc else []
    bad += ['gather bank %d: %s' % (k, m) for k in range(nseg) for m in [differ(host(outs[k]), banks[k].numpy()[gi[:n]])] if m and not rc]
    bad += ['stash %s' % host(stash).tolist()] if host(stash).tolist() != [77, -5, 123456] else []
    si = tc.scatter_rows(n, rows, nseg)
    srcs = [tc.rows_data(n, v, 'msrc%d' % k) for k, v in enumerate(lens)]
    dsts = [guarded.alloc((rows, v), torch.float32, DEV) for v in lens]
    rc = L().usot_rows_copy_multi_f32(st(), nseg, pp([guarded.put(s, DEV) for s in srcs]), P(guarded.put(torch.from_numpy(si), DEV)),
                                      pp(dsts), n, rl, 1, None)
    bad += ['scatter: return code %d' % rc] if rc else []
    bad += ['scatter bank %d: %s' % (k, m) for k in range(nseg) for m in [differ(host(dsts[k]), rows_expected_scatter(srcs[k], si, rows))]
            if m and not rc]
    finish('rows_copy_multi past the cap, row lengths %s' % lens, start, 2, bad)


# ============================================================================================================ batch append + gather
def test_append_gather_batch_rows_out_of_range():
    """usot_rows_append_gather_batch_f32 with picks and append rows at -1, bank_rows, INT32_MIN and INT32_MAX beside in-range slots in
    one launch: such an append is dropped, such a pick gathers zeros - also a pick that EQUALS its slot's out-of-range append_row -
    and no bank row but the two in-range append rows changes."""
    start = guarded.registry_size()
    a = tc.AG
    fresh = [tc.rows_data(a['B'], n, 'fresh%d' % k) for k, n in enumerate(a['lens'])]
    banks = [tc.rows_data(a['bank_rows'], n, 'bank%d' % k) for k, n in enumerate(a['lens'])]
    want_banks, want_picked = tc.ag_ref(fresh, banks)
    ctl, recs = ctl_block(a['B'], 9.0)
    for b in range(a['B']):
        recs[b]['append_row'] = a['append'][b]
        recs[b]['picks'][:a['n_pick']] = a['picks'][b]
        recs[b]['picks'][a['n_pick']:] = tc.INT32_MAX          # never read
    dbanks = [guarded.put(t, DEV) for t in banks]
    picked = [guarded.alloc((a['B'] * a['n_pick'], n), torch.float32, DEV) for n in a['lens'][1:]]
    pp = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    rc = L().usot_rows_append_gather_batch_f32(st(), pp([guarded.put(t, DEV) for t in fresh]), pp(dbanks), pp(picked),
                                               (C.c_int32 * 4)(*a['lens']), P(guarded.put(torch.from_numpy(ctl), DEV)), a['B'], a['n_pick'],
                                               a['bank_rows'])
    bad = ['return code %d' % rc] if rc else []
    bad += ['bank %d: %s' % (k, m) for k in range(4) for m in [differ(host(dbanks[k]), want_banks[k].numpy())] if m]
    bad += ['picked %d: %s' % (k + 1, m) for k in range(3) for m in [differ(host(picked[k]), want_picked[k].numpy())] if m]
    finish('append + gather, rows out of range', start, 1, bad)
