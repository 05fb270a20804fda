"""The canary checker of tests/guarded.py, tested on CPU tensors through the `whole` tensor of a guarded allocation: this is
where its sensitivity is shown (no GPU kernel is ever made to overrun on purpose)."""
import types

import pytest
import torch

import guarded
from guarded import GUARD_BYTES


@pytest.fixture(autouse=True)
def _clean_registry():
    guarded._registry.clear()
    yield
    guarded._registry.clear()


def test_layout_guard_sizes_and_alignment():
    t = guarded.alloc((3, 5), torch.float32)
    w = guarded.whole_of(t)
    assert GUARD_BYTES == 64 * 1024 and GUARD_BYTES % 512 == 0
    assert w.dtype == torch.uint8 and w.numel() == 2 * GUARD_BYTES + 60
    assert t.data_ptr() - w.data_ptr() == GUARD_BYTES                       # front guard, then the interior
    assert t.is_contiguous() and tuple(t.shape) == (3, 5)
    front, rear = w[:GUARD_BYTES].view(torch.int16), w[GUARD_BYTES + 60:].view(torch.int16)
    assert rear.numel() * 2 == GUARD_BYTES                                  # rear guard starts at the first byte after the interior
    assert bool((front == 0x7FC1).all()) and bool((rear == 0x7FC1).all())


def test_untouched_run_passes():
    t = guarded.alloc((7, 9), torch.float32)
    u = guarded.alloc((11,), torch.bfloat16, prefill='zero')
    v = guarded.alloc((5,), torch.uint8)                                     # odd byte count: the rear guard is not 2-byte aligned
    t.copy_(torch.randn(7, 9))
    u.fill_(1.0)
    v.fill_(255)
    t[-1, -1] = 3.0                                                          # the last element of the interior is not the guard
    t[0, 0] = 4.0
    assert guarded.registry_size() == 3
    guarded.check()
    assert guarded.registry_size() == 0


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.uint8])
def test_one_element_before_the_interior_is_reported(dtype):
    t = guarded.alloc((4, 6), dtype)
    es = t.element_size()
    w = guarded.whole_of(t)
    w[GUARD_BYTES - es:GUARD_BYTES].view(dtype)[0] = 1                       # element -1
    with pytest.raises(guarded.GuardError) as e:
        guarded.check()
    msg = str(e.value)
    assert 'front guard' in msg and 'rear guard' not in msg
    assert 'first at byte offset %d,' % -es in msg and 'last at -1 ' in msg
    assert '(4, 6)' in msg and str(dtype).replace('torch.', '') in msg and 'test_guarded_host.py' in msg


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.uint8])
@pytest.mark.parametrize('shape', [(4, 6), (3, 5, 1), (7,)])
def test_one_element_after_the_interior_is_reported(dtype, shape):
    t = guarded.alloc(shape, dtype)
    es, nb = t.element_size(), t.numel() * t.element_size()
    w = guarded.whole_of(t)
    w[GUARD_BYTES + nb:GUARD_BYTES + nb + es] = torch.zeros(es, dtype=torch.uint8)      # element numel: a zero, say
    with pytest.raises(guarded.GuardError) as e:
        guarded.check()
    msg = str(e.value)
    assert 'rear guard' in msg and 'front guard' not in msg
    assert 'first at byte offset %d,' % nb in msg and 'last at %d ' % (nb + es - 1) in msg
    assert str(shape) in msg and 'test_guarded_host.py' in msg


def test_a_row_written_past_the_end_names_first_and_last_byte():
    t = guarded.alloc((5, 8), torch.float32)
    w = guarded.whole_of(t)
    w[GUARD_BYTES + 160:GUARD_BYTES + 160 + 32].view(torch.float32)[:] = torch.arange(1, 9, dtype=torch.float32)      # row 5 of 5
    far = guarded.alloc((2,), torch.float32)
    guarded.whole_of(far)[-1] = 0                                             # the very last byte of a rear guard counts too
    with pytest.raises(guarded.GuardError) as e:
        guarded.check()
    msg = str(e.value)
    assert 'first at byte offset 160, last at 191 ' in msg
    assert 'first at byte offset %d, last at %d ' % (8 + GUARD_BYTES - 1, 8 + GUARD_BYTES - 1) in msg
    assert msg.startswith('2 guard(s) damaged')


def test_writing_the_canary_value_itself_is_invisible_but_any_other_bit_is_not():
    t = guarded.alloc((3,), torch.float16)
    w = guarded.whole_of(t)
    w[GUARD_BYTES + 6:GUARD_BYTES + 10].view(torch.int16).fill_(guarded.CANARY)     # a stray store of the pattern: not seen (a fixed condition)
    w[GUARD_BYTES - 2:GUARD_BYTES].view(torch.int16).fill_(guarded.CANARY)
    guarded.check(clear=False)
    w[GUARD_BYTES + 6] ^= 1                                                  # one bit of the first rear byte
    with pytest.raises(guarded.GuardError):
        guarded.check()


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16])
def test_unwritten_interior_element_is_nan(dtype):
    t = guarded.alloc((6, 7), dtype)                                          # prefill 'canary': what `empty` means
    assert bool(torch.isnan(t).all())
    t.copy_(torch.ones(6, 7))
    t2 = guarded.alloc((6, 7), dtype)
    t2[:, :6] = 1.0                                                           # a kernel that skips the last column
    assert int(torch.isnan(t2).sum()) == 6 and bool(torch.isnan(t2[:, 6]).all())
    assert not bool(torch.isfinite(t2.float().sum()))
    z = guarded.alloc((6, 7), dtype, prefill='zero')
    assert not z.any()
    f = guarded.alloc((6, 7), dtype, prefill='full', fill_value=2.5)
    assert bool((f == 2.5).all())
    guarded.check()


def test_odd_fp32_element_count_is_nan_to_the_last_element():
    t = guarded.alloc((5,), torch.float32)
    assert bool(torch.isnan(t).all())
    assert t.view(torch.int32).tolist() == [0x7FC17FC1] * 5


def test_put_keeps_values_and_strides_and_unchanged_detects_a_bit():
    x = torch.randn(2, 6, 4, 5)
    g = guarded.put(x)
    assert torch.equal(g, x) and g.stride() == x.stride()
    cl = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)               # channels-last view (what prroi_pool takes)
    gc = guarded.put(cl)
    assert torch.equal(gc, cl) and gc.stride() == cl.stride() and not gc.is_contiguous()
    with pytest.raises(ValueError):
        guarded.put(x[:, ::2])                                                # not dense
    snap = guarded.snapshot(g)
    guarded.unchanged(g, snap)
    g.view(torch.int32)[1, 2, 3, 4] ^= 1                                      # the lowest mantissa bit of one element
    with pytest.raises(guarded.GuardError) as e:
        guarded.unchanged(g, snap, 'x')
    assert 'x of shape (2, 6, 4, 5) was modified: 1 bytes differ' in str(e.value)
    n = torch.tensor([float('nan'), 1.0])
    guarded.unchanged(n, guarded.snapshot(n))                                 # bitwise: a NaN equals itself
    guarded.check()


def _module_using_torch():
    m = types.ModuleType('fake_wrappers')
    m.torch = torch
    exec('def out(shape, device, dtype=None):\n'
         '    return torch.empty(shape, device=device, dtype=dtype or torch.float32)\n'
         'def short(rows, cols, device):\n'
         '    return torch.empty((rows - 1, cols), device=device, dtype=torch.float32)\n', m.__dict__)
    return m


def test_proxy_delegates_everything_it_does_not_intercept():
    p = guarded.TorchProxy()
    assert p.float32 is torch.float32 and p.Tensor is torch.Tensor and p.cuda is torch.cuda and p.nn is torch.nn
    assert p.device('cpu') == torch.device('cpu')
    a = p.randn(3)
    assert type(a) is torch.Tensor and isinstance(a, p.Tensor)
    before = guarded.registry_size()
    for t in (p.empty(3, 4), p.zeros((3, 4), dtype=torch.float64), p.full((2,), 1.5), p.empty(5, device='cpu'),
              p.empty_like(a), p.zeros_like(a), p.full_like(a, 2.0), p.zeros(6, dtype=torch.uint8)):
        assert type(t) is torch.Tensor
    assert guarded.registry_size() == before                                  # CPU allocations are left alone
    assert p.zeros(2, 3, dtype=torch.int32).tolist() == [[0, 0, 0], [0, 0, 0]] and p.full((2,), 7).dtype == torch.int64
    with pytest.raises(AttributeError):
        p.empty = None


def test_proxy_leaves_pinned_requests_to_torch():
    """pin_memory=True is torch's business (it needs a device runtime; here only the routing is checked)."""
    p = guarded.TorchProxy()
    assert not p._on_device(None, False) and not p._on_device('cpu', False) and not p._on_device('cuda:0', True)
    assert p._on_device('cuda:0', False) and p._on_device(torch.device('cuda', 1), False)


def test_proxy_routes_device_allocations_through_alloc(monkeypatch):
    """Stand-in for the device: alloc() is told 'meta'-free CPU memory, the routing decision is forced."""
    p = guarded.TorchProxy('canary')
    monkeypatch.setattr(guarded.TorchProxy, '_on_device', staticmethod(lambda device, pin: not pin))
    e = p.empty((2, 3), device='cpu', dtype=torch.float32)
    z = p.zeros(4, device='cpu')
    f = p.full((3,), 7, device='cpu')
    el = p.empty_like(torch.ones(2, 2, dtype=torch.bfloat16))
    fl = p.full_like(torch.ones(3), 0.5)
    cl = p.zeros_like(torch.ones(2, 3, 4, 5).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
    assert guarded.registry_size() == 6
    assert bool(torch.isnan(e).all()) and not z.any() and f.tolist() == [7, 7, 7] and f.dtype == torch.int64
    assert bool(torch.isnan(el).all()) and el.dtype == torch.bfloat16 and fl.tolist() == [0.5] * 3
    assert cl.stride() == (60, 1, 15, 3) and not cl.any()
    assert not bool(torch.isnan(guarded.TorchProxy('zero').empty(3, device='cpu')).any())
    with pytest.raises(TypeError):
        p.empty(3, device='cpu', memory_format=torch.contiguous_format)
    guarded.check()


def test_patched_swaps_the_name_checks_on_exit_and_restores(monkeypatch):
    monkeypatch.setattr(guarded.TorchProxy, '_on_device', staticmethod(lambda device, pin: not pin))
    m = _module_using_torch()
    with guarded.patched(m) as proxy:
        assert m.torch is proxy
        y = m.out((3, 4), 'cpu')
        assert bool(torch.isnan(y).all()) and guarded.registry_size() == 1
        y.fill_(1.0)
    assert m.torch is torch and guarded.registry_size() == 0
    with guarded.patched(m, empty_prefill='zero'):
        assert not m.out((3, 4), 'cpu').any()
    with pytest.raises(ZeroDivisionError):                                    # the test's own failure is not masked, the name is restored
        with guarded.patched(m):
            m.out((2,), 'cpu')
            1 / 0
    assert m.torch is torch and guarded.registry_size() == 0


def test_an_allocation_one_row_short_fails_with_its_call_site(monkeypatch):
    """A wrapper that allocates one row too few while the 'kernel' stores the full shape: the stores of the last row land in
    the rear guard, and the report names the wrapper's line."""
    monkeypatch.setattr(guarded.TorchProxy, '_on_device', staticmethod(lambda device, pin: not pin))
    m = _module_using_torch()
    rows, cols = 6, 10
    with pytest.raises(guarded.GuardError) as e:
        with guarded.patched(m):
            y = m.short(rows, cols, 'cpu')
            flat = guarded.whole_of(y)[GUARD_BYTES:GUARD_BYTES + rows * cols * 4].view(torch.float32)     # what the kernel is told
            flat.copy_(torch.arange(rows * cols, dtype=torch.float32))
    msg = str(e.value)
    assert 'rear guard of float32 (5, 10)' in msg and 'in short' in msg
    assert 'first at byte offset 200, last at 239 ' in msg
