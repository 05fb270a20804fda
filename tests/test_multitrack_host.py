"""CPU: lock-step multi-video tracking without a GPU - the batched entry points of csrc/multitrack.hip are declared, exported
and check their arguments; the BatchSession's host bookkeeping (engine.SlotBook) packs the step's control block as
include/usot_hip.h lays it out; track_dataset schedules more videos than slots and gives every video exactly the `regions`
of the reference's one-video-after-another loop (scripts/test_usot.py:72-105)."""
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest
import torch

from usot_amd import build, hip
from usot_amd.engine import IDLE_TSZ, SLOT_REC, STEP_HDR, MemoryBank, SlotBook, crop_fields, wait_tags
from usot_amd.hostutils import crop_geometry
from usot_amd.io_utils import cxy_wh_2_rect, get_axis_aligned_bbox, poly_iou
from usot_amd.multitrack import track_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('usot_decode_batch_f32', 'usot_plan_add_decode_batch', 'usot_rows_append_gather_batch_f32',
       'usot_plan_add_rows_append_gather_batch', 'usot_crop_resize_batch_u8_f32', 'usot_plan_add_crop_resize_batch')
EINVAL = -1


@pytest.fixture(scope='module')
def L():
    build.build(force=False)
    return hip.lib()


def test_batched_entry_points_are_exported_and_check_their_arguments(L):
    with open(os.path.join(ROOT, 'include', 'usot_hip.h')) as f:
        declared = set(re.findall(r'\b(usot_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)))
    raw = C.CDLL(hip.LIB_PATH)
    for s in NEW:
        assert s in declared and s in hip.EXPORTS and hasattr(raw, s), s
    assert L.usot_abi_version() == 6
    fake = C.c_void_p(0x1000)              # recorded by the adders, never dereferenced: nothing is launched here
    f4 = (C.c_void_p * 4)(*[0x1000] * 4)
    f3 = (C.c_void_p * 3)(*[0x1000] * 3)
    rl = (C.c_int32 * 4)(7 * 7 * 256, 5 * 5 * 256, 3 * 5 * 256, 5 * 3 * 256)
    plan = C.c_void_p(L.usot_plan_create())
    try:
        def dec(B=4, S=25, cls=fake, out=fake, ctl=fake, roi=fake):
            return L.usot_plan_add_decode_batch(plan, cls, fake, fake, fake, out, B, S, 255, 8, C.c_float(0.3), C.c_double(0.021),
                                                C.c_double(0.321), ctl, roi)

        def ag(B=4, nq=7, fresh=f4, picked=f3, lens=rl, ctl=fake, rows=4096):
            return L.usot_plan_add_rows_append_gather_batch(plan, fresh, f4, picked, lens, ctl, B, nq, rows)

        def crop(B=4, S=255, ctl=fake, out=fake):
            return L.usot_plan_add_crop_resize_batch(plan, ctl, out, B, S)

        for bad in (dict(B=0), dict(B=-3), dict(S=33), dict(S=0), dict(cls=None), dict(out=None), dict(ctl=None), dict(roi=None)):
            assert dec(**bad) == EINVAL, bad
        for bad in (dict(B=0), dict(nq=0), dict(nq=33), dict(ctl=None), dict(fresh=None), dict(rows=0),
                    dict(picked=(C.c_void_p * 3)(0x1000, None, 0x1000)), dict(lens=(C.c_int32 * 4)(12544, 6, 3840, 3840))):
            assert ag(**bad) == EINVAL, bad
        for bad in (dict(B=0), dict(S=0), dict(ctl=None), dict(out=None)):
            assert crop(**bad) == EINVAL, bad
        assert L.usot_plan_size(plan) == 0
        assert dec() == 0 and dec(B=32, S=27) == 0 and ag() == 0 and ag(nq=32) == 0 and crop() == 0
        assert L.usot_plan_size(plan) == 5
        assert L.usot_plan_add_decode_batch(None, fake, fake, fake, fake, fake, 4, 25, 255, 8, C.c_float(0.3), C.c_double(0.021),
                                            C.c_double(0.321), fake, fake) == EINVAL
    finally:
        L.usot_plan_destroy(plan)
    # the eager entry points check before they launch
    assert L.usot_decode_batch_f32(None, fake, fake, fake, fake, fake, 0, 25, 255, 8, C.c_float(0.3), C.c_double(0.021),
                                   C.c_double(0.321), fake, fake) == EINVAL
    assert L.usot_decode_batch_f32(None, fake, fake, fake, fake, fake, 2, 33, 255, 8, C.c_float(0.3), C.c_double(0.021),
                                   C.c_double(0.321), fake, fake) == EINVAL
    assert L.usot_rows_append_gather_batch_f32(None, f4, f4, f3, rl, fake, 4, 33, 4096) == EINVAL
    assert L.usot_rows_append_gather_batch_f32(None, f4, f4, f3, rl, None, 4, 7, 4096) == EINVAL
    assert L.usot_crop_resize_batch_u8_f32(None, fake, fake, 0, 255) == EINVAL
    assert L.usot_crop_resize_batch_u8_f32(None, None, fake, 2, 255) == EINVAL


def test_control_block_packing():
    assert SLOT_REC.itemsize == 192
    assert [SLOT_REC.fields[k][1] for k in ('tsz', 'im', 'H', 'W', 'x0', 'y0', 'win', 'fill', 'append_row', 'next_row', 'picks')] \
        == [0, 16, 24, 28, 32, 36, 40, 44, 56, 60, 64]
    B, cap, nq = 4, 16, 7
    book = SlotBook(B, cap, nq)
    ctl = np.zeros(STEP_HDR + B * SLOT_REC.itemsize, np.uint8)
    recs = ctl[STEP_HDR:].view(SLOT_REC)
    scratch = [b * cap + cap - 1 for b in range(B)]
    book.load(1)
    book.load(2)
    # the crop record: the window origin in image coordinates and the truncated fill of Session.frame_from_image
    im_shape, pos, win, avg = (360, 480, 3), (30.4, 300.2), 301, np.array([12.7, 99.2, 200.9])
    cf = crop_fields(im_shape, pos, win, avg)
    (cx0, _, cy0, _), (top, _, left, _) = crop_geometry(im_shape, pos, win)
    assert cf == (int(cx0) - left, int(cy0) - top, 301, (12, 99, 200))
    book.pack(recs, {1: ([0] * 5, (40.0, 30.0)), 2: ([0] * 5, (10.0, 12.0))}, {1: (0xdead0000, 360, 480) + cf})
    # first step after a load: nothing pending, every append goes to the slot's scratch row; global rows are b * cap + r
    assert [int(r) for r in recs['append_row']] == scratch
    assert list(recs[1]['picks'][:nq]) == [16, 17, 18, 18, 18, 18, 18] and set(recs[1]['picks'][nq:]) == {scratch[1]}
    assert list(recs[2]['picks'][:nq]) == [32, 33, 34, 34, 34, 34, 34]
    assert recs[1]['next_row'] == 16 + 3 and tuple(recs[1]['tsz']) == (40.0, 30.0)
    assert int(recs[1]['im']) == 0xdead0000 and (recs[1]['H'], recs[1]['W'], recs[1]['x0'], recs[1]['y0'], recs[1]['win']) \
        == (360, 480) + cf[:3] and tuple(recs[1]['fill']) == cf[3]
    assert int(recs[2]['im']) == 0                      # a crop the host writes itself
    for b in (0, 3):                                    # inactive slots: no crop, everything on the scratch row
        assert int(recs[b]['im']) == 0 and set(recs[b]['picks']) == {scratch[b]} and recs[b]['next_row'] == scratch[b]
        assert tuple(recs[b]['tsz']) == IDLE_TSZ
    book.stepped({1: None, 2: None})
    assert book.n[1] == book.n[2] == 2 and book.pending[1] and book.prev_row[1] == 19
    # slot 2 sits the next step out: its pending feature still lands (the step's PrRoIPool overwrites the pooled buffer)
    book.pack(recs, {1: ([0, 0, 0, 1, 1], (40.0, 30.0))})
    assert recs[1]['append_row'] == 19 and recs[2]['append_row'] == 35
    assert list(recs[1]['picks'][:nq]) == [16, 17, 18, 18, 18, 19, 19]
    assert int(recs[2]['im']) == 0 and set(recs[2]['picks']) == {scratch[2]}
    book.stepped({1: None})
    assert not book.pending[2] and book.prev_row[2] == scratch[2] and book.n[2] == 2 and book.n[1] == 3
    # a new video in slot 1: the previous occupant's pending append goes to the scratch row
    assert book.pending[1]
    book.load(1)
    book.pack(recs, {1: ([0] * 5, (1.0, 1.0))})
    assert recs[1]['append_row'] == scratch[1] and recs[1]['next_row'] == 16 + 3
    with pytest.raises(ValueError):                     # picks name stored memory features only
        book.pack(recs, {1: ([0, 0, 0, 0, 1], (1.0, 1.0))})
    with pytest.raises(ValueError):
        book.pack(recs, {0: ([0] * 5, (1.0, 1.0))})      # slot 0 holds no video
    book.release(2)
    assert book.free_slot() == 0 and not book.active[2]
    # growth doubles every slot's region: rows move to b * 2cap + r
    book.n[1] = 13
    assert book.need_grow()
    book.grow()
    assert book.cap == 32 and book.row(3, 5) == 101 and book.scratch(1) == 63 and not book.need_grow()


# ---------------------------------------------------------------------------------------------------- track_dataset
LOST = {('v2', 4), ('v5', 8)}            # (video, frame) where the scripted tracker loses the target


def _move(state, im):
    """The scripted tracker: a per-video drift, or a jump far outside the frame at the frames of LOST."""
    if (im['vid'], im['f']) in LOST:
        pos = np.array([5000.0, 5000.0])
    else:
        pos = state['target_pos'] + np.array([1.0 + 0.25 * int(im['vid'][1:]), 0.5])
    return dict(target_pos=pos, target_sz=state['target_sz'] * 1.01)


class StubTracker(object):
    """MultiVideoTracker's interface over _move; counts the videos it holds at once."""

    def __init__(self, slots):
        self.slots, self.states, self.next, self.most, self.adds = slots, {}, 0, 0, []

    def add(self, im, target_pos, target_sz):
        assert len(self.states) < self.slots
        key, self.next = self.next, self.next + 1
        self.states[key] = dict(target_pos=np.asarray(target_pos, np.float64), target_sz=np.asarray(target_sz, np.float64))
        self.most = max(self.most, len(self.states))
        self.adds.append((im['vid'], im['f']))
        return key

    def track(self, frames):
        assert 0 < len(frames) <= self.slots
        for key, im in frames.items():
            self.states[key] = _move(self.states[key], im)
        return {key: self.states[key] for key in frames}

    def remove(self, key):
        del self.states[key]


def _imread(fn):
    return dict(vid=fn[0], f=fn[1])


def _dataset():
    out = {}
    for i, n in enumerate((7, 3, 12, 5, 9, 10)):
        name = 'v%d' % i
        gt = [np.array([40.0 + (1.0 + 0.25 * i) * f, 30.0 + 0.5 * f, 20.0, 16.0]) for f in range(n)]
        out[name] = {'image_files': [(name, f) for f in range(n)], 'gt': gt, 'name': name}
    return out


def _sequential(dataset, vot):
    """scripts/test_usot.py:72-105, one video after another, with the scripted tracker."""
    out = {}
    for name, video in dataset.items():
        start_frame, regions, state = 0, [], None
        for f, image_file in enumerate(video['image_files']):
            im = _imread(image_file)
            if f == start_frame:
                cx, cy, w, h = get_axis_aligned_bbox(video['gt'][f])
                state = dict(target_pos=np.array([cx, cy]), target_sz=np.array([w, h]))
                regions.append(1 if vot else video['gt'][f])
            elif f > start_frame:
                state = _move(state, im)
                location = cxy_wh_2_rect(state['target_pos'], state['target_sz'])
                b_overlap = poly_iou(video['gt'][f], location) if vot else 1
                if b_overlap > 0:
                    regions.append(location)
                else:
                    regions.append(2)
                    start_frame = f + 5
            else:
                regions.append(0)
        out[name] = regions
    return out


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(y, int):
            assert isinstance(x, int) and x == y, (x, y)
        else:
            assert np.array_equal(np.asarray(x, np.float64), np.asarray(y, np.float64)), (x, y)


@pytest.mark.parametrize('vot', [False, True], ids=['ope', 'vot'])
def test_track_dataset_schedules_like_the_sequential_loop(vot):
    ds = _dataset()
    stub = StubTracker(slots=2)
    got = track_dataset(None, ds, slots=2, imread=_imread, vot=vot, tracker=stub)
    want = _sequential(ds, vot)
    assert list(got) == list(ds)
    for name in ds:
        _same(got[name], want[name])
        assert len(got[name]) == len(ds[name]['image_files'])
    assert stub.most == 2 and not stub.states          # both slots used, every video released at its end
    # slots are refilled as videos end: v2 starts while v0 still runs, and every video was added
    assert [a for a in stub.adds if a[1] == 0] == [('v%d' % i, 0) for i in range(6)]
    if vot:
        assert got['v2'][4:10] == [2, 0, 0, 0, 0, 1] and stub.adds.count(('v2', 9)) == 1    # lost, 0 x 4, re-init 5 frames later
        assert got['v5'][8:] == [2, 0]                                                       # lost too late to re-init
        assert all(not isinstance(r, int) for r in got['v0'][1:])
    else:
        assert all(not isinstance(r, int) for name in ds for r in got[name][1:])
    # one slot: the same regions again
    got1 = track_dataset(None, ds, slots=1, imread=_imread, vot=vot, tracker=StubTracker(slots=1))
    for name in ds:
        _same(got1[name], want[name])


@pytest.mark.parametrize('slots', [1, 3])
def test_memory_bank_growth_keeps_every_slots_rows(slots):
    """engine.MemoryBank.grow on CPU tensors: after one doubling old row r of slot b sits at b * 8 + r with its values, the new
    rows are zero; at slots = 1 that is the single session's copy (the first `cap` rows unchanged, zeros behind them)."""
    bank = MemoryBank(slots, 4, 'cpu')
    tensors = [bank.feat] + bank.enc
    for t in tensors:
        assert t.shape[0] == slots * 4
        for b in range(slots):
            for r in range(4):
                t[b * 4 + r] = float(b * 100 + r)
    before = [t.clone() for t in tensors]
    bank.grow()
    assert bank.cap == 8
    for old, t in zip(before, [bank.feat] + bank.enc):
        assert tuple(t.shape) == (slots * 8,) + tuple(old.shape[1:]) and t.dtype == old.dtype
        for b in range(slots):
            assert torch.equal(t[b * 8:b * 8 + 4], old[b * 4:b * 4 + 4])
            assert torch.equal(t[b * 8:b * 8 + 4], torch.stack([torch.full(old.shape[1:], float(b * 100 + r)) for r in range(4)]))
            assert not t[b * 8 + 4:b * 8 + 8].any()
        if slots == 1:
            want = torch.zeros_like(t)
            want[:4].copy_(old)
            assert torch.equal(t, want)
    ptrs, lens = bank.marshal()
    assert list(ptrs) == [t.data_ptr() for t in [bank.feat] + bank.enc] and list(lens) == [7 * 7 * 256, 5 * 5 * 256, 3 * 5 * 256, 5 * 3 * 256]


class _Stream(object):
    syncs = 0

    def synchronize(self):
        self.syncs += 1


def test_wait_tags_three_stages():
    """engine.wait_tags on a numpy tag array: tags that are there return at once; tags that arrive after the spin budget are
    found by the sleeping polls; tags that never arrive synchronise the stream once and raise with the tag and the value read."""
    st = _Stream()
    words = np.full(3, 7.0)
    wait_tags(words, 7.0, st, 0.001)
    assert st.syncs == 0
    words[:] = 6.0
    timer = threading.Timer(0.01, lambda: words.fill(7.0))
    timer.start()
    try:
        wait_tags(words, 7.0, st, 0.001)
    finally:
        timer.join()
    assert st.syncs == 0 and (words == 7.0).all()
    words[:] = [8.0, 8.0, 5.0]
    with pytest.raises(hip.HipError) as ei:
        wait_tags(words, 8.0, st, 0.001, deadline=0.05)
    assert st.syncs == 1
    assert str(ei.value) == ('frame 8.0 never published its result block (tag reads 5.0): '
                             'the frame graph did not run to the decode kernel')
