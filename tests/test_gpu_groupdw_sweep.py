"""GPU: every GroupDW kernel variant at every geometry its launcher accepts - the eleven cols_per_thread codes behind
usot_groupdw_multi_f32 (csrc/xcorr.hip), the 16-bit outputs of usot_groupdw_multi_lp and the run-time sample count of
usot_groupdw_multi_dyn_f32 - against the float64 reference of tests/groupdw_cases.py.

  G   geometry per variant: patch and strip residues in both axes and non-square both ways (1, 5, 50, 52), column groups (2), every
      accepted width with its ragged last strip (3, 4), all residues of the five-way unrolled row loop (6 - 9); auto (cols 0) below
      and at 64 samples, checked against usot_groupdw_auto_variant as well.
  C   the `C != 256` block mapping: 64 .. 512 channels x 1, 2, 5 samples on every code.
  S   three segments of 3 + 2 + 5 samples with x_rep 1, 2, 3 (at C = 256 the sample pairs (2, 3) and (4, 5) straddle both borders)
      and two segments of one sample, on every code at C = 256 and 128.
  D   pixel strides and channel offsets: the engine's merged maps, per-branch values, and odd values where a variant loads by dwords.
  L   usot_groupdw_multi_lp, fp16 and bf16.
  Y   usot_groupdw_multi_dyn_f32 with counts below 0, inside and above the capacity of the last segment.
  P   the persistent kernels (8, 9) with unit counts around one and two rounds of the resident grid.
  B   normal-distributed operands: 6 - 9 agree bit for bit, 16-bit outputs are the rounding of variant 6's, every code is within the
      existing rel_err < 1e-5 of float64.
  R   everything the launcher refuses: USOT_EINVAL and every output's bits untouched.

Operands of G, C, S, D, L, Y, P are exact (groupdw_cases.py), so every comparison there is EQUALITY: bit for bit in fp32 and fp16,
the round-to-nearest-even in bf16.  Outputs are NaN-prefilled between canaries (tests/guarded.py), inputs lie between NaNs, the
channels of a strided operand outside its slice are NaN, every test ends with guarded.check.

One item = one (part, code); it loops over its list and reports every failing case, not the first one.  The lists are asserted by
tests/test_groupdw_lists.py."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import groupdw_cases as gw  # noqa: E402
import guarded  # noqa: E402
from test_gpu_ops import rel_err  # noqa: E402
from usot_amd import hip  # noqa: E402

DEV = 'cuda:0'
EINVAL = -1
LP = [pytest.param(torch.float16, 1, id='fp16'), pytest.param(torch.bfloat16, 2, id='bf16')]
CODE = [pytest.param(c, id='v%d' % c) for c in gw.CODES]


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def put_segments(segs):
    """guarded device copies of every segment's operands: [(three maps, three templates)]"""
    return [([guarded.put(t, DEV) for t in g.x], [guarded.put(t, DEV) for t in g.z]) for g in segs]


def new_outs(case, segs, dtype=torch.float32):
    return [guarded.alloc((g.S, case.OH, case.OW, case.C), dtype, DEV) for g in segs]


def descriptors(case, segs, dev, outs, cols=None, last_s=None):
    arr = (hip.GroupDWDesc * max(len(segs), 1))()
    for k, (g, (xd, zd), o) in enumerate(zip(segs, dev, outs)):
        S = last_s if last_s is not None and k == len(segs) - 1 else g.S
        arr[k] = hip.groupdw_desc([t.data_ptr() for t in xd], [t.data_ptr() for t in zd], o.data_ptr(), g.wsm, S=S, x_rep=g.x_rep,
                                  OH=case.OH, OW=case.OW, Cc=case.C, x_cs=g.x_cs, x_co=g.x_co, z_cs=g.z_cs, z_co=g.z_co,
                                  cols=case.cols if cols is None else cols)
    return arr


def launch(arr, nseg, out_dtype=0, count=None):
    if count is not None:
        return hip.lib().usot_groupdw_multi_dyn_f32(hip.stream(), arr, nseg, count)
    if out_dtype:
        return hip.lib().usot_groupdw_multi_lp(hip.stream(), arr, nseg, out_dtype)
    return hip.lib().usot_groupdw_multi_f32(hip.stream(), arr, nseg)


def mismatch(out, want):
    """'' when the device tensor holds exactly the bits of `want` (a CPU tensor of the output's type), else what differs"""
    want = want.to(DEV)
    if same_bits(out, want):
        return ''
    ne = bits(out) != bits(want)
    first = ne.reshape(-1).nonzero()[0].item()
    idx = []
    for n in reversed(out.shape):
        idx.insert(0, first % n)
        first //= n
    return '%d of %d elements differ (%d NaN), first at [s, i, j, c] = %s: got %r, want %r' % (
        int(ne.sum()), out.numel(), int(torch.isnan(out).sum()), idx, float(out[tuple(idx)]), float(want[tuple(idx)]))


def run_exact(case, dtype=torch.float32, out_dtype=0):
    """one launch of a case of parts G, C, S, D, L -> failure texts"""
    segs, refs = gw.build(case)
    outs = new_outs(case, segs, dtype)
    rc = launch(descriptors(case, segs, put_segments(segs), outs), len(segs), out_dtype)
    if rc != 0:
        return ['return code %d' % rc]
    return ['segment %d: %s' % (k, m) for k, (o, ref) in enumerate(zip(outs, refs)) for m in [mismatch(o, gw.stored(ref, dtype))] if m]


def sweep(part, what, cases, **kw):
    start = guarded.registry_size()
    bad = []
    for case in cases:
        bad += [(tuple(case), m) for m in run_exact(case, **kw)]
    torch.cuda.synchronize()
    guarded.check(start)
    print('%s %s: %d launches, %d failing' % (part, what, len(cases), len(bad)))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- G, C, S, D
@pytest.mark.parametrize('code', CODE)
def test_g_every_geometry(code):
    """G.  One segment of three samples, C = 64, every (OH, OW) of the variant's list."""
    sweep('G', 'variant %d' % code, gw.g_cases(code))


def test_g_auto():
    """G.  cols_per_thread 0 below 64 samples and at 64 samples (OW 25 with and without shared maps, OW 23): right, and the variant
    usot_groupdw_auto_variant names is the specified one."""
    for case, variant in gw.auto_cases():
        assert hip.lib().usot_groupdw_auto_variant(sum(s for s, _ in case.segs), case.OW) == variant, case
    sweep('G', 'auto', [c for c, _ in gw.auto_cases()])


@pytest.mark.parametrize('code', CODE)
def test_c_every_channel_count(code):
    """C.  64, 128, 192, 256, 320, 512 channels x 1, 2, 5 samples."""
    sweep('C', 'variant %d' % code, gw.c_cases(code))


@pytest.mark.parametrize('code', CODE)
def test_s_segments(code):
    """S.  Three segments (3, 2, 5 samples; x_rep 1, 2, 3) and two segments of one sample at C = 256 and 128; every segment has its
    own maps, templates, weights and output."""
    sweep('S', 'variant %d' % code, gw.s_cases(code))


@pytest.mark.parametrize('code', CODE)
def test_d_strides_and_offsets(code):
    """D.  Merged maps (either half), per-branch strides and offsets, odd values where the variant loads by dwords."""
    sweep('D', 'variant %d' % code, gw.d_cases(code))


# ------------------------------------------------------------------------------------------------------------------------- L
@pytest.mark.parametrize('dtype,code', LP)
def test_l_sixteen_bit_outputs(dtype, code):
    """L.  usot_groupdw_multi_lp: fp16 outputs equal the float64 value, bf16 outputs its round-to-nearest-even."""
    sweep('L', str(dtype), gw.l_cases(), dtype=dtype, out_dtype=code)


# ------------------------------------------------------------------------------------------------------------------------- Y
@pytest.mark.parametrize('case', gw.y_cases(), ids=lambda c: 'c%d' % c.C)
def test_y_run_time_count(case):
    """Y.  Counts -3, 0, 1, 4, 5, 9 on a last segment of capacity 5: clamp(count, 0, 5) samples are live, bit-equal to the static
    launch and equal to float64; the rest keeps its prefill bits."""
    start = guarded.registry_size()
    segs, refs = gw.build(case)
    dev = put_segments(segs)
    cnt = guarded.alloc((1,), torch.int32, DEV, 'zero')
    bad = []
    for count in gw.Y_COUNTS:
        live = min(max(count, 0), gw.Y_CAPACITY)
        want = new_outs(case, segs)
        hip.check(launch(descriptors(case, segs, dev, want, last_s=live or None), 3 if live else 2), 'static launch')
        got = new_outs(case, segs)
        blank = got[2].clone()
        cnt.fill_(count)
        hip.check(launch(descriptors(case, segs, dev, got), 3, count=hip.ptr(cnt)), 'run-time count')
        for k in range(2):
            bad += [(count, k, m) for m in [mismatch(got[k], refs[k].float())] if m]
            bad += [(count, k, 'differs from the static launch')] if not same_bits(got[k], want[k]) else []
        bad += [(count, 2, m) for m in [mismatch(got[2][:live], refs[2][:live].float())] if m]
        bad += [(count, 2, 'live samples differ from the static launch')] if not same_bits(got[2][:live], want[2][:live]) else []
        bad += [(count, 2, 'a sample past the count was written')] if not same_bits(got[2][live:], blank[live:]) else []
    torch.cuda.synchronize()
    guarded.check(start)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------- P
@pytest.mark.parametrize('oh', gw.P_OH)
@pytest.mark.parametrize('ow', gw.P_OW)
def test_p_persistent_rounds(ow, oh):
    """P.  Variants 8 and 9 with the unit count one step below, at and above the resident grid, and above two rounds of it; x_rep 3,
    so neighbouring units read different maps.  One set of operands per channel count: a launch of n samples reads its first n
    templates and ceil(n / 3) maps, and owes the first n samples of the reference."""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    bad, launches = [], 0
    for Cc, counts in gw.p_counts(cu).items():
        start = guarded.registry_size()
        case = gw.p_case(oh, ow, Cc, max(counts))
        g = gw.segment(oh, ow, Cc, max(counts), gw.P_XREP, 0)
        ref = gw.ref64(g, oh, ow, Cc).float().to(DEV)
        dev = put_segments([g])
        for n in counts:
            for code in gw.PERSISTENT:
                out = guarded.alloc((n, oh, ow, Cc), torch.float32, DEV)
                rc = launch(descriptors(case, [g], dev, [out], cols=code, last_s=n), 1)
                launches += 1
                if rc != 0 or not same_bits(out, ref[:n]):
                    bad.append((Cc, n, code, 'return code %d' % rc if rc else mismatch(out, ref[:n])))
        torch.cuda.synchronize()
        guarded.check(start)
    print('P %dx%d on %d CUs (resident grid %d): %d launches, %d failing' % (oh, ow, cu, gw.p_resident(cu), launches, len(bad)))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize('case', gw.b_cases(), ids=lambda c: '%dx%d_c%d' % (c.OH, c.OW, c.C))
def test_b_real_valued_operands(case):
    """B.  Normal-distributed operands, three segments: every code within rel_err < 1e-5 of float64; 6, 7, 8, 9 bit-identical (same
    arithmetic in the same order); the 16-bit outputs are variant 6's values rounded once."""
    start = guarded.registry_size()
    segs, refs = gw.build(case, True)
    dev = put_segments(segs)
    res, bad = {}, []
    for code in gw.CODES:
        res[code] = new_outs(case, segs)
        hip.check(launch(descriptors(case, segs, dev, res[code], cols=code), 3), 'variant %d' % code)
    lp = {}
    for dtype, dt in ((torch.float16, 1), (torch.bfloat16, 2)):
        lp[dtype] = new_outs(case, segs, dtype)
        hip.check(launch(descriptors(case, segs, dev, lp[dtype]), 3, dt), 'lp %s' % dtype)
    torch.cuda.synchronize()
    guarded.check(start)
    for k, ref in enumerate(refs):
        for code in gw.CODES:
            err = rel_err(res[code][k].cpu().numpy(), ref.numpy())
            if not err < 1e-5:
                bad.append((code, k, 'rel_err %.3g' % err))
        for code in (7, 8, 9):
            if not same_bits(res[code][k], res[6][k]):
                bad.append((code, k, '%d elements differ from variant 6' % int((res[code][k] != res[6][k]).sum())))
        for dtype, o in lp.items():
            if not same_bits(o[k], res[6][k].to(dtype)):
                ne = int((bits(o[k]) != bits(res[6][k].to(dtype))).sum())
                bad.append((str(dtype), k, '%d of %d elements are not the rounding of variant 6' % (ne, o[k].numel())))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------- R
def _rejection(row):
    """build a launch the launcher accepts, make the one change the row names, launch: -> (return code, outputs untouched)"""
    name, entry, code, OH, OW, what, arg = row
    nseg = 2 if what == 'seg2' else 1
    case = gw.Case('R', code, OH, OW, 64, gw.ONE * max(nseg, 4 if what == 'nseg' else 1), 'dense')
    segs, _ = gw.build(case)
    dev = put_segments(segs)
    outs = new_outs(case, segs)
    snaps = [guarded.snapshot(o) for o in outs]
    arr = descriptors(case, segs, dev, outs)
    out_dtype, count = 0, None
    if entry == 'dyn':
        word = guarded.alloc((2,), torch.int32, DEV, 'full', 1)
        count = C.c_void_p(word.data_ptr())
    if what == 'field':
        setattr(arr[0], arg[0], arg[1])
    elif what == 'seg2':
        setattr(arr[1], arg[0], arg[1])
    elif what == 'elem':
        getattr(arr[0], arg[0])[arg[1]] = arg[2]
    elif what == 'advance':
        getattr(arr[0], arg[0])[arg[1]] += arg[2]
    elif what == 'nseg':
        nseg = arg
    elif what == 'out_dtype':
        out_dtype = arg
    elif what == 'count_advance':
        count = C.c_void_p(word.data_ptr() + arg)
    else:
        assert what is None, what
    if entry == 'lp':
        rc = hip.lib().usot_groupdw_multi_lp(hip.stream(), arr, nseg, out_dtype)
    else:
        rc = launch(arr, nseg, 0, count)
    torch.cuda.synchronize()
    return rc, all(torch.equal(guarded.snapshot(o), s) for o, s in zip(outs, snaps))


def test_r_rejections():
    """R.  Every refusal of the launcher: USOT_EINVAL, nothing written."""
    start = guarded.registry_size()
    bad = []
    rows = gw.r_cases()
    for row in rows:
        rc, untouched = _rejection(row)
        if rc != EINVAL or not untouched:
            bad.append((row[0], 'return code %d' % rc, 'outputs untouched' if untouched else 'AN OUTPUT WAS WRITTEN'))
    guarded.check(start)
    print('R: %d refusals, %d failing' % (len(rows), len(bad)))
    assert not bad, bad


def test_r_rows_are_accepted_without_their_change():
    """the launches of part R differ from an accepted launch in the named change only: each base launch (same entry point, code and
    geometry, nothing changed) is accepted wherever the code and geometry themselves are not the refusal"""
    start = guarded.registry_size()
    bad, seen = [], set()
    for name, entry, code, OH, OW, what, arg in gw.r_cases():
        if what is None or (entry, code, OH, OW) in seen or (entry == 'lp' and OW == 26):
            continue
        seen.add((entry, code, OH, OW))
        out_dtype = 1 if entry == 'lp' else 0
        base = 'dyn' if entry == 'dyn' else 'f32'
        rc, _ = _rejection((name, base if not out_dtype else 'lp', code, OH, OW, 'out_dtype' if out_dtype else None, out_dtype or None))
        if rc != 0:
            bad.append((name, 'the unchanged launch returns %d' % rc))
    guarded.check(start)
    assert seen and not bad, bad
