"""The optimiser of the reference's training loop on the HIP side: SGD with momentum, dampening, weight decay and Nesterov over
every parameter group in ONE launch of csrc/sgd.hip, with the reference's `if is_valid_number(loss.item()): optimizer.step()`
moved onto the device (no host synchronisation) and, on request, `zero_grad()` folded into the same pass.

    opt = SGD(groups, lr=..., momentum=0.9, weight_decay=1e-4, zero_grads=True)
    loss.backward()
    opt.step(loss=loss)          # skipped on the device when the loss is NaN, +-Inf or > 1e4

There is no CPU path: parameters and gradients must be dense fp32 device tensors (hip.HipError otherwise).  The state layout
(`state[p]['momentum_buffer']`) and the group keys are torch.optim.SGD's, so state dicts load either way."""
import math
import operator

import numpy as np
import torch
from torch.optim.optimizer import Optimizer

from . import hip

GUARD_MAX = 1e4
_RECORD = np.dtype({'names': [f[0] for f in hip.SgdTensor._fields_],
                    'formats': ['u8', 'u8', 'u8', 'i8', 'f4', 'f4', 'f4', 'f4', 'i4', 'i4'],
                    'offsets': [getattr(hip.SgdTensor, f[0]).offset for f in hip.SgdTensor._fields_],
                    'itemsize': hip.C.sizeof(hip.SgdTensor)})


def is_valid_number(x):
    """The reference's lib/utils/train_utils.py:is_valid_number - the host form of the guard csrc/sgd.hip applies to the loss."""
    return not (math.isnan(x) or math.isinf(x) or x > GUARD_MAX)


class SGD(Optimizer):
    """torch.optim.SGD's constructor and state, one HIP launch per step.  `foreach`, `differentiable` and `fused` are accepted and
    kept in `defaults` for state-dict compatibility only.  zero_grads: the step stores 0 over every gradient it read (applied or
    skipped), which replaces the loop's zero_grad()."""

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None, zero_grads=False):
        if isinstance(lr, torch.Tensor) and lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused)
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, defaults)
        self.zero_grads = bool(zero_grads)
        self.uploads = 0                 # table images sent to the device so far
        self._unborn = {}                # parameter -> zeroed buffer whose first step the guard skipped: not yet in `state`
        self._plan = None                # what _steady() needs of the last fully validated step
        self._stage = self._stage_np = self._table = self._sent = self._counters = None
        self._shape = (0, 0)             # (T, n_chunks) of the uploaded image

    def __setstate__(self, state):
        super().__setstate__(state)
        for name, value in (('zero_grads', False), ('uploads', 0), ('_unborn', {}), ('_plan', None), ('_stage', None), ('_stage_np', None),
                            ('_table', None), ('_sent', None), ('_counters', None), ('_shape', (0, 0))):
            self.__dict__.setdefault(name, value)            # an unpickled optimiser holds defaults, state and groups only
        for group in self.param_groups:
            group.setdefault('nesterov', False)
            group.setdefault('maximize', False)
            group.setdefault('foreach', None)
            group.setdefault('differentiable', False)
            group.setdefault('fused', None)

    def zero_grad(self, set_to_none=False):
        """Keeps the gradient tensors by default, so their addresses - and the uploaded table - stay as they are; they are zeroed
        in one multi-tensor pass per device and type.  (With zero_grads=True the step has done it already.)"""
        if set_to_none:
            return super().zero_grad(set_to_none=True)
        by_kind = {}
        for group in self.param_groups:
            for p in group['params']:
                g = p.grad
                if g is not None:
                    if g.grad_fn is not None:
                        g.detach_()
                    else:
                        g.requires_grad_(False)
                    by_kind.setdefault((g.device, g.dtype), []).append(g)
        for grads in by_kind.values():
            torch._foreach_zero_(grads)

    def counters(self):
        """(steps applied, steps skipped by the guard) so far, read from the device: a synchronisation."""
        if self._counters is None:
            return (0, 0)
        applied, skipped = self._counters.tolist()
        return (applied, skipped)

    def _records(self):
        """One record per parameter that has a gradient, from the groups' current hyper-parameters, every tensor validated ->
        (structured array, [(parameter, buffer)] of the records whose first-step flag is set, device).  Leaves
        the plan _steady() works from, unless some tensor is on its first step."""
        cols = {k: [] for k in _RECORD.names if k != 'reserved'}
        first, gidx, tensors, states, bufs = [], [], [], [], []
        device = None
        for k, group in enumerate(self.param_groups):
            lr, mu, wd = float(group['lr']), float(group['momentum']), float(group['weight_decay'])
            scale = 1.0 - float(group['dampening'])
            base = (hip.SGD_NESTEROV if group['nesterov'] else 0) | (hip.SGD_MAXIMIZE if group['maximize'] else 0)
            for p in group['params']:
                g = p.grad
                if g is None:
                    continue
                for what, t in (('parameter', p), ('gradient', g)):
                    if not (t.is_cuda and t.dtype == torch.float32 and t.layout == torch.strided and t.is_contiguous()):
                        raise hip.HipError('SGD.step: a %s of shape %s is not a dense fp32 device tensor (the HIP step has no CPU '
                                           'implementation)' % (what, tuple(t.shape)))
                if g.shape != p.shape or (device is not None and (p.device != device or g.device != device)):
                    raise hip.HipError('SGD.step: parameters and gradients must agree in shape and sit on one device')
                device = p.device
                flags, buf = base, None
                tensors += [p, g]
                if mu != 0:
                    state = self.state[p]
                    buf = state.get('momentum_buffer')
                    if buf is None:
                        buf = self._unborn.get(p)
                        if buf is None:
                            buf = self._unborn[p] = torch.zeros_like(p)
                        flags |= hip.SGD_FIRST
                        first.append((p, buf))
                    elif not (buf.is_cuda and buf.dtype == torch.float32 and buf.is_contiguous() and buf.shape == p.shape
                              and buf.device == device):
                        raise hip.HipError('SGD.step: the momentum buffer of a parameter of shape %s is not a dense fp32 device tensor'
                                           % (tuple(p.shape),))
                    tensors.append(buf)
                    states.append(state)
                    bufs.append(buf)
                gidx.append(k)
                cols['p'].append(p.data_ptr())
                cols['g'].append(g.data_ptr())
                cols['buf'].append(buf.data_ptr() if buf is not None else 0)
                cols['n'].append(p.numel())
                cols['lr'].append(lr)
                cols['weight_decay'].append(wd)
                cols['momentum'].append(mu)
                cols['grad_scale'].append(scale)             # formed in double, rounded to fp32 once by the assignment below
                cols['flags'].append(flags)
        rec = np.zeros(len(cols['p']), dtype=_RECORD)
        for k, v in cols.items():
            rec[k] = v
        self._plan = None
        if len(rec) and not first:
            every = [p for group in self.param_groups for p in group['params']]
            self._plan = dict(state=self.state, groups=self.param_groups, lists=[(g['params'], len(g['params'])) for g in self.param_groups],
                              mom=[g['momentum'] != 0 for g in self.param_groups], every=every, grads=[p.grad for p in every],
                              states=states, bufs=bufs, tensors=tensors, ptrs=[t.data_ptr() for t in tensors], rec=rec,
                              gidx=np.array(gidx, dtype=np.intp), device=device)
        return rec, first, device

    def _steady(self):
        """The records of a step over the very tensors of the last one - the same groups and lists, the same gradient and buffer
        objects at the same addresses, still dense (which _records validated in full) - with the groups' CURRENT hyper-parameters:
        the steady state of a training loop, without 234 rounds of checks.  None when anything moved: _records starts over."""
        pl = self._plan
        if pl is None or self.state is not pl['state'] or self.param_groups is not pl['groups'] or len(pl['groups']) != len(pl['lists']):
            return None
        for group, (params, count), mom in zip(pl['groups'], pl['lists'], pl['mom']):
            if group['params'] is not params or len(params) != count or (group['momentum'] != 0) != mom:
                return None
        if not all(map(operator.is_, [p.grad for p in pl['every']], pl['grads'])):
            return None
        if not all(map(operator.is_, [st.get('momentum_buffer') for st in pl['states']], pl['bufs'])):
            return None
        if list(map(torch.Tensor.data_ptr, pl['tensors'])) != pl['ptrs'] or not all(map(torch.Tensor.is_contiguous, pl['tensors'])):
            return None
        hyper = np.array([[float(g['lr']), float(g['weight_decay']), float(g['momentum']), 1.0 - float(g['dampening']),
                           (hip.SGD_NESTEROV if g['nesterov'] else 0) | (hip.SGD_MAXIMIZE if g['maximize'] else 0)]
                          for g in pl['groups']], dtype=np.float64)[pl['gidx']]
        rec = pl['rec']
        rec['lr'], rec['weight_decay'], rec['momentum'], rec['grad_scale'], rec['flags'] = hyper.T
        return rec, [], pl['device']

    def _upload(self, image, shape, device):
        """Send the image unless it is, byte for byte, the one the device holds."""
        new = np.frombuffer(image, dtype=np.uint8)
        if self._sent is not None and shape == self._shape and self._table.device == device and np.array_equal(new, self._stage_np):
            return
        if self._sent is not None:
            self._sent.synchronize()         # the previous copy has left the staging tensor
        if self._stage is None or self._stage.numel() != new.size or self._table.device != device:
            self._stage = torch.empty(new.size, dtype=torch.uint8, pin_memory=True)
            self._stage_np = self._stage.numpy()
            self._table = torch.empty(new.size, dtype=torch.uint8, device=device)
        self._stage_np[:] = new
        self._table.copy_(self._stage, non_blocking=True)
        self._sent = torch.cuda.Event()
        self._sent.record(torch.cuda.current_stream(device))
        self._shape = shape
        self.uploads += 1

    @torch.no_grad()
    def step(self, closure=None, *, loss=None):
        """One step.  loss: a one-element fp32 device tensor, the guard - read on the device, never synchronised, except on a step
        that is some tensor's first: there the host has to learn whether its buffer was initialised."""
        result = None
        if closure is not None:
            with torch.enable_grad():
                result = closure()
        if loss is not None:
            if not (isinstance(loss, torch.Tensor) and loss.is_cuda and loss.dtype == torch.float32 and loss.numel() == 1):
                raise hip.HipError('SGD.step: the guard must be a one-element fp32 device tensor')
            loss = loss.detach()
        rec, first, device = self._steady() or self._records()
        if not len(rec):
            return result
        if loss is not None and loss.device != device:
            raise hip.HipError('SGD.step: the guard sits on %s, the parameters on %s' % (loss.device, device))
        with torch.cuda.device(device):
            image, n_chunks = hip.sgd_table((hip.SgdTensor * len(rec)).from_buffer(rec))
            self._upload(image, (len(rec), n_chunks), device)
            if self._counters is None or self._counters.device != device:
                self._counters = torch.zeros(2, dtype=torch.int32, device=device)
            applied = True
            if first and loss is not None:
                before = self._counters.tolist()[0]
            hip.sgd_step(self._table, len(rec), n_chunks, guard=loss, counters=self._counters, zero_grads=self.zero_grads)
            if first and loss is not None:
                applied = self._counters.tolist()[0] != before
        if applied:
            for p, buf in first:
                self.state[p]['momentum_buffer'] = buf
                self._unborn.pop(p, None)
        return result
