"""Lock-step multi-video tracking: `MultiVideoTracker` steps many videos through ONE frame graph per instance size
(engine.BatchSession), and `track_dataset` runs a `benchmarks.load_dataset` dict through it, producing per video exactly the
`regions` list of the reference's one-video-after-another loop (scripts/test_usot.py:40-105).

Per video the host logic is USOTTracker.track's fused path: select_memory on the video's own confidences, the decoded box
applied with _apply_box, the clamps.  Decoded frames: `track_dataset` reads images with Pillow by default (cv2 is not a
dependency), so its pixels are Pillow's JPEG decode, which is not pinned to cv2's.
"""
import numpy as np
import torch

from .hostutils import python2round
from .io_utils import cxy_wh_2_rect, get_axis_aligned_bbox, poly_iou
from .tracker import USOTTracker, search_scale, select_memory

# slots per instance size (videos stepped together); DESIGN.md section 6 has the measurement behind the choice
DEFAULT_SLOTS = 4


class _Info(object):
    arch = 'USOT'
    dataset = 'USOT'
    epoch_test = False


class MultiVideoTracker(object):
    """Many videos, one lock-step graph launch per instance size and step.

    add(im, target_pos, target_sz) -> key   USOTTracker.init for one more video (it takes a free slot)
    track({key: im}) -> {key: state}        one step of the listed videos; the others sit it out
    state(key) / remove(key)

    A video's state dict has USOTTracker's keys; `target_pos` / `target_sz` are read from it at every step (callers may
    teacher-force or re-initialise), `memory_features` is a MemoryFeatures view of the slot's bank rows."""

    def __init__(self, info, model, slots=None, backbone_dtype=torch.float32, capacity=1024):
        self.info, self.model = info, model
        self.slots = int(slots or DEFAULT_SLOTS)
        self.backbone_dtype = backbone_dtype
        self.capacity = int(capacity)
        self._init = USOTTracker(info)
        self._sessions = {}          # instance size -> BatchSession
        self._videos = {}            # key -> (state, session, slot)
        self._next = 0

    def session(self, instance_size):
        return self._sessions.get(int(instance_size))

    def add(self, im, target_pos, target_sz):
        from .engine import MemoryFeatures, SlotMemory
        state = self._init.init_state(im, target_pos, target_sz, self.model)
        p = state['p']
        bs = self._sessions.get(int(p.instance_size))
        if bs is None:
            bs = self.model.engine.open_batch_session(p, state['window'], self.slots, capacity=self.capacity,
                                                      backbone_dtype=self.backbone_dtype)
            self._sessions[int(p.instance_size)] = bs
        slot = bs.book.free_slot()
        if slot is None:
            raise RuntimeError('all %d slots of instance size %d hold a video' % (self.slots, p.instance_size))
        bs.load(slot, self.model.zf, state['init_features'])
        state['session'] = bs
        state['memory_features'] = MemoryFeatures(SlotMemory(bs, slot))
        key = self._next
        self._next += 1
        self._videos[key] = (state, bs, slot)
        return key

    def state(self, key):
        return self._videos[key][0]

    def slot(self, key):
        return self._videos[key][2]

    def remove(self, key):
        _, bs, slot = self._videos.pop(key)
        bs.release(slot)

    def __len__(self):
        return len(self._videos)

    def track(self, frames):
        groups, pre = {}, {}
        for key, im in frames.items():
            state, bs, slot = self._videos[key]
            p = state['p']
            target_pos, target_sz = state['target_pos'], state['target_sz']
            s_x, scale_z = search_scale(target_sz, p)
            picks = select_memory(USOTTracker._conf_array(state, state['memory_confidences']), p.mem_queue_size)
            tsz = target_sz * scale_z
            groups.setdefault(id(bs), (bs, {}))[1][slot] = dict(image=im, pos=target_pos, win=python2round(s_x),
                                                                 avg_chans=state['avg_chans'], picks=picks, tsz=tsz)
            pre[key] = (scale_z, tsz)
        for bs, items in groups.values():            # every graph on its way before the first wait
            bs.submit(items)
        outs = {g: bs.collect() for g, (bs, _) in groups.items()}
        res = {}
        for key in frames:
            state, bs, slot = self._videos[key]
            scale_z, tsz = pre[key]
            USOTTracker._apply_result(state, outs[id(bs)][slot], tsz, scale_z)
            res[key] = state
        return res


def pil_imread(path):
    """BGR uint8 [H,W,3] with Pillow (grayscale expanded to three channels, as test_usot.py does with cv2.cvtColor)."""
    from PIL import Image
    with Image.open(path) as im:
        rgb = np.asarray(im.convert('RGB'))
    return np.ascontiguousarray(rgb[:, :, ::-1])


class _Run(object):
    """One video's pass of the test_usot.py loop: frame cursor, re-init frame, regions, tracker key."""

    def __init__(self, name, video):
        self.name, self.files, self.gt = name, video['image_files'], video['gt']
        self.f, self.start, self.regions, self.key = 0, 0, [], None


def track_dataset(model, dataset, slots=None, imread=None, vot=False, tracker=None, info=None):
    """{name: regions} of every video of `dataset` (a load_dataset dict), tracked in lock step: up to `slots` videos at a time,
    a slot refilled with the next video as soon as one ends.  regions per video as scripts/test_usot.py:72-105 builds them:
    the init frame gives its gt box (1 for VOT), a tracked frame cxy_wh_2_rect of the state; VOT: an overlap <= 0 gives 2,
    then 0 until the re-init 5 frames later.  `tracker`: an object with MultiVideoTracker's add / track / remove
    (default: MultiVideoTracker(info, model, slots))."""
    imread = imread or pil_imread
    slots = int(slots or DEFAULT_SLOTS)
    mt = tracker if tracker is not None else MultiVideoTracker(info or _Info(), model, slots)
    queue = list(dataset)
    running, results = [], {}

    def advance(r):
        """Init and skipped frames up to the next frame that needs a step; False when the video has ended."""
        while r.f < len(r.files):
            f = r.f
            if f == r.start:
                im = imread(r.files[f])
                cx, cy, w, h = get_axis_aligned_bbox(r.gt[f])
                if r.key is not None:
                    mt.remove(r.key)
                r.key = mt.add(im, np.array([cx, cy]), np.array([w, h]))
                r.regions.append(1 if vot else r.gt[f])
            elif f > r.start:
                return True
            else:
                r.regions.append(0)
            r.f += 1
        return False

    def finish(r):
        if r.key is not None:
            mt.remove(r.key)
            r.key = None
        results[r.name] = r.regions

    while queue or running:
        while queue and len(running) < slots:
            name = queue.pop(0)
            r = _Run(name, dataset[name])
            if advance(r):
                running.append(r)
            else:
                finish(r)
        if not running:
            continue
        states = mt.track({r.key: imread(r.files[r.f]) for r in running})
        still = []
        for r in running:
            st = states[r.key]
            location = cxy_wh_2_rect(st['target_pos'], st['target_sz'])
            overlap = poly_iou(r.gt[r.f], location) if vot else 1
            if overlap > 0:
                r.regions.append(location)
            else:
                r.regions.append(2)
                r.start = r.f + 5
                mt.remove(r.key)
                r.key = None
            r.f += 1
            if advance(r):
                still.append(r)
            else:
                finish(r)
        running = still
    return {name: results[name] for name in dataset}
