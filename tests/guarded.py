"""Canary allocations: every tensor handed out here is the interior of a larger allocation with 64 KiB of a fixed bit pattern in
front of it and 64 KiB behind it.  A kernel that stores outside its output damages a guard (check() names the allocation, the
side and the damaged bytes); a kernel that skips an element, or reads one nobody wrote, meets the same pattern inside the
interior, where it decodes as NaN in bf16, fp16 and (as a pair) fp32.

Plain helper module: no fixtures, no pytest hooks.  The guards lie inside the same allocation as the interior, so nothing here
touches memory the process does not own.  What a guard cannot see: a read outside an input that does not reach the result,
and a write that starts more than 64 KiB away from the interior."""
import contextlib
import os
import traceback

import torch as _torch

GUARD_BYTES = 64 * 1024                     # a multiple of 512 B: the interior keeps the caching allocator's alignment
CANARY = 0x7FC1                             # bf16 NaN, fp16 NaN; 0x7FC17FC1 is an fp32 NaN
_LO, _HI = CANARY & 0xFF, CANARY >> 8       # little-endian bytes of the pattern

_HERE = os.path.abspath(__file__)
_registry = []                              # one record per live guarded allocation


class GuardError(AssertionError):
    pass


def _call_site():
    for fr in reversed(traceback.extract_stack()[:-1]):
        if os.path.abspath(fr.filename) != _HERE and 'contextlib' not in fr.filename:
            return '%s:%d in %s' % (os.path.relpath(fr.filename, os.path.dirname(os.path.dirname(_HERE))), fr.lineno, fr.name)
    return '?'


def _pattern_fill(u8):
    """Fill a uint8 slice with the canary, phase 0 at its first byte."""
    n = u8.numel()
    if u8.storage_offset() % 2 == 0 and n % 2 == 0:
        u8.view(_torch.int16).fill_(CANARY)
    else:
        u8[0::2] = _LO
        u8[1::2] = _HI


def _damage(u8):
    """Boolean per byte of a guard slice: differs from the canary (phase 0 at the slice's first byte).  For the report."""
    want = _torch.empty_like(u8)
    want[0::2] = _LO
    want[1::2] = _HI
    return u8 != want


def _touched(u8):
    """0-d boolean tensor: any bit of a guard slice differs from the canary.  Compared as int16; a rear guard behind an interior of
    an odd number of bytes is not 2-byte aligned and is compared byte by byte."""
    if u8.storage_offset() % 2 == 0 and u8.numel() % 2 == 0:
        return (u8.view(_torch.int16) != CANARY).any()
    return _damage(u8).any()


def alloc(shape, dtype=_torch.float32, device='cpu', prefill='canary', fill_value=None, site=None):
    """Interior view [shape] of a guarded allocation.  prefill: 'canary' (what `empty` means: any bits, here the NaN pattern),
    'zero', 'full' (fill_value) or 'none' (the caller fills it)."""
    if isinstance(shape, int):
        shape = (shape,)
    shape = tuple(int(s) for s in shape)
    n = 1
    for s in shape:
        n *= s
    nbytes = n * _torch.empty(0, dtype=dtype).element_size()
    whole = _torch.empty(2 * GUARD_BYTES + nbytes, dtype=_torch.uint8, device=device)
    _pattern_fill(whole[:GUARD_BYTES])
    _pattern_fill(whole[GUARD_BYTES + nbytes:])                   # starts at the first byte after the interior: no slack
    inner = whole[GUARD_BYTES:GUARD_BYTES + nbytes]
    if prefill == 'canary':
        if nbytes:
            _pattern_fill(inner)
    elif prefill == 'zero':
        inner.zero_()
    elif prefill not in ('full', 'none'):
        raise ValueError('prefill %r' % (prefill,))
    interior = (inner.view(dtype) if nbytes else _torch.empty(0, dtype=dtype, device=whole.device)).view(shape)
    if prefill == 'full':
        interior.fill_(fill_value)
    _registry.append({'whole': whole, 'interior': interior, 'nbytes': nbytes, 'shape': shape, 'dtype': dtype,
                      'site': site or _call_site()})
    return interior


def whole_of(t):
    """The uint8 tensor (front guard | interior | rear guard) an interior belongs to."""
    for r in _registry:
        if r['interior'] is t:
            return r['whole']
    raise KeyError('not a guarded allocation')


def _is_dense(t):
    """Non-overlapping strides that cover exactly numel elements (a permutation of a contiguous tensor)."""
    dims = sorted(((st, sz) for st, sz in zip(t.stride(), t.shape) if sz != 1))
    want = 1
    for st, sz in dims:
        if st != want:
            return False
        want *= sz
    return True


def put(t, device=None):
    """Guarded device copy of an input tensor: a NaN on both sides of it.  Dense tensors keep their strides (a channels-last view
    of an NHWC buffer is copied as that buffer and the view re-applied)."""
    device = device if device is not None else t.device
    site = _call_site()
    if t.is_contiguous() or t.numel() == 0:
        g = alloc(t.shape, t.dtype, device, 'none', site=site)
        g.copy_(t)
        return g
    if not _is_dense(t):
        raise ValueError('put: strides %s of shape %s are not dense' % (t.stride(), tuple(t.shape)))
    flat = alloc((t.numel(),), t.dtype, device, 'none', site=site)
    g = flat.as_strided(t.shape, t.stride())
    g.copy_(t)
    return g


def snapshot(t):
    """Bit copy of a tensor's elements, for unchanged()."""
    return _bits(t).clone()


def _bits(t):
    t = t.detach().contiguous()
    return t.view(_torch.uint8) if t.numel() else t.reshape(-1)


def unchanged(t, snap, what='input'):
    """Assert that `t` is bit-identical to snapshot(t) taken before the call."""
    now = _bits(t)
    if not _torch.equal(now, snap):
        bad = (now.reshape(-1) != snap.reshape(-1)).nonzero().reshape(-1)
        raise GuardError('%s of shape %s was modified: %d bytes differ, first at byte %d, last at byte %d'
                         % (what, tuple(t.shape), bad.numel(), int(bad[0]), int(bad[-1])))


def registry_size():
    return len(_registry)


def _report(r):
    out = []
    nb = r['nbytes']
    for side, u8 in (('front', r['whole'][:GUARD_BYTES]), ('rear', r['whole'][GUARD_BYTES + nb:])):
        bad = _damage(u8).nonzero().reshape(-1)
        if bad.numel():
            first, last = int(bad[0]), int(bad[-1])
            if side == 'front':             # offsets relative to the interior: negative in front of it, from nbytes on behind it
                first, last = first - GUARD_BYTES, last - GUARD_BYTES
            else:
                first, last = first + nb, last + nb
            out.append('%s guard of %s %s allocated at %s damaged: %d bytes, first at byte offset %d, last at %d of an interior of %d bytes'
                       % (side, str(r['dtype']).replace('torch.', ''), r['shape'], r['site'], bad.numel(), first, last, nb))
    return out


def check(start=0, clear=True):
    """Assert that every guard of the allocations registered from index `start` on is untouched; forget them when `clear`."""
    recs = _registry[start:]
    try:
        if not recs:
            return
        flags = [_touched(r['whole'][:GUARD_BYTES]) | _touched(r['whole'][GUARD_BYTES + r['nbytes']:]) for r in recs]
        by_dev = {}
        for f in flags:
            by_dev.setdefault(f.device, []).append(f)
        if any(bool(_torch.stack(fs).any()) for fs in by_dev.values()):      # one synchronisation per device
            msgs = []
            for r in recs:
                msgs += _report(r)
            raise GuardError('%d guard(s) damaged:\n  ' % len(msgs) + '\n  '.join(msgs))
    finally:
        if clear:
            del _registry[start:]


class TorchProxy(object):
    """Stands in for the name `torch` inside a module: the six allocation functions go through alloc() when the result is a device
    tensor; every other attribute is the real torch's."""

    def __init__(self, empty_prefill='canary'):
        if empty_prefill not in ('canary', 'zero'):
            raise ValueError(empty_prefill)
        object.__setattr__(self, '_prefill', empty_prefill)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        raise AttributeError('the torch proxy is read-only')

    @staticmethod
    def _shape(args):
        if len(args) == 1 and not isinstance(args[0], int):
            return tuple(args[0])
        return tuple(args)

    @staticmethod
    def _on_device(device, pin):
        return device is not None and not pin and _torch.device(device).type != 'cpu'

    def _make(self, real, shape, prefill, fill_value, kw, args):
        device, dtype, pin = kw.get('device'), kw.get('dtype'), kw.get('pin_memory', False)
        if not self._on_device(device, pin):
            return real(*args, **kw)
        extra = set(kw) - {'device', 'dtype', 'pin_memory', 'requires_grad'}
        if extra:
            raise TypeError('guarded torch proxy: unsupported arguments %s for a device allocation' % sorted(extra))
        if dtype is None:
            if prefill == 'full' and isinstance(fill_value, bool):
                dtype = _torch.bool
            elif prefill == 'full' and isinstance(fill_value, int):
                dtype = _torch.int64
            else:
                dtype = _torch.get_default_dtype()
        t = alloc(shape, dtype, device, prefill, fill_value, site=_call_site())
        return t.requires_grad_(True) if kw.get('requires_grad') else t

    def empty(self, *args, **kw):
        return self._make(_torch.empty, self._shape(args), self._prefill, None, kw, args)

    def zeros(self, *args, **kw):
        return self._make(_torch.zeros, self._shape(args), 'zero', None, kw, args)

    def full(self, size, fill_value, **kw):
        return self._make(_torch.full, tuple(size), 'full', fill_value, kw, (size, fill_value))

    def _like(self, real, t, prefill, fill_value, kw, args):
        device = kw.get('device', t.device)
        if not self._on_device(device, kw.get('pin_memory', False)):
            return real(*args, **kw)
        extra = set(kw) - {'device', 'dtype', 'requires_grad'}
        if extra:
            raise TypeError('guarded torch proxy: unsupported arguments %s for a device allocation' % sorted(extra))
        if t.numel() and not t.is_contiguous():
            if not _is_dense(t):
                raise TypeError('guarded torch proxy: *_like of a tensor with non-dense strides')
            flat = alloc((t.numel(),), kw.get('dtype', t.dtype), device, prefill, fill_value, site=_call_site())
            out = flat.as_strided(t.shape, t.stride())         # preserve_format, as torch does for dense tensors
        else:
            out = alloc(t.shape, kw.get('dtype', t.dtype), device, prefill, fill_value, site=_call_site())
        return out.requires_grad_(True) if kw.get('requires_grad') else out

    def empty_like(self, t, **kw):
        return self._like(_torch.empty_like, t, self._prefill, None, kw, (t,))

    def zeros_like(self, t, **kw):
        return self._like(_torch.zeros_like, t, 'zero', None, kw, (t,))

    def full_like(self, t, fill_value, **kw):
        return self._like(_torch.full_like, t, 'full', fill_value, kw, (t, fill_value))


@contextlib.contextmanager
def patched(*modules, **kw):
    """Inside the block the name `torch` of each given module is a TorchProxy(empty_prefill); on a clean exit every guard
    allocated inside the block is checked.  The modules themselves are not edited."""
    proxy = TorchProxy(kw.pop('empty_prefill', 'canary'))
    if kw:
        raise TypeError('patched: unexpected arguments %s' % sorted(kw))
    start = len(_registry)
    saved = [(m, m.torch) for m in modules]
    for m in modules:
        m.torch = proxy
    try:
        yield proxy
    except BaseException:
        del _registry[start:]
        raise
    finally:
        for m, real in saved:
            m.torch = real
    check(start)
