"""Name -> optimizer (torchdet3d/builders/optim_builder.py:3-19; 'adam' builds AdamW, :10-12).  The model exposes
ONE flat parameter (all weights, see models/engine.py), so every optimizer here is a single elementwise update over
~2.4-4.4 M floats instead of ~190 small tensors.  All four names are hand-written HIP kernels (csrc/misc.hip:
`t3d_adamw_step`, `t3d_sgd_step`, `t3d_rmsprop_step`, `t3d_adadelta_step`) behind the torch.optim.Optimizer interface --
same hyper-parameters, same state-dict layout and LR-scheduler behaviour as the torch.optim class of that name, so
checkpoints cross both ways -- and all four run inside the step plan (trainer/step_plan.py).  A parameter that is not on
the GPU gets the framework optimizer, as does a user who builds one by hand; that one takes the eager form of the step."""
import torch

from .. import _native as N

AVAILABLE_OPTIMS = ['sgd', 'rmsprop', 'adam', 'adadelta']


class FusedOptimizer(torch.optim.Optimizer):
    """What the four kernel optimizers share: one HIP launch per parameter tensor, `grad_scale` multiplied into the gradient on
    load (1/world after a summed all-reduce), the divergence watch, and torch's checkpoint form.  A subclass names its entry
    point and state buffers (`_buffers`), its hyper-parameters in call order (`_hyper`), and issues the launch (`_call`).
    `ensure_state` / `plan_key` / `launch` / `advance` are the whole interface the step plan uses (trainer/step_plan.py), so
    `step()` and the plan share one launch site."""

    def __init__(self, params, defaults, grad_scale=1.0):
        super().__init__(params, defaults)
        self.grad_scale = grad_scale
        self._watch = None            # device int64: the first step that met a non-finite gradient (t3d_set_grad_watch)

    def watch_word(self, device):
        if self._watch is None or self._watch.device != torch.device(device):
            self._watch = torch.full((1,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=device)
        return self._watch

    def first_nonfinite_step(self):
        """The 1-based optimizer step whose gradient was the first to hold an inf / NaN, or None (one 8-byte read-back and a
        wait: call it where the loop waits anyway)."""
        if self._watch is None:
            return None
        v = int(self._watch.item())
        return None if v == torch.iinfo(torch.int64).max else v

    # ---- per optimizer
    def _buffers(self, group):
        """Names of the per-parameter state tensors (torch's names), in the entry point's argument order."""
        raise NotImplementedError

    def _hyper(self, group):
        """The hyper-parameters other than `lr` that the launch reads: changing one re-records a step plan."""
        raise NotImplementedError

    def _call(self, p, grad, st, group, stream, slots):
        raise NotImplementedError

    # ---- what step() and the step plan are made of
    def _group(self, p):
        for g in self.param_groups:
            if any(q is p for q in g['params']):
                return g
        raise KeyError('parameter is not in this optimizer')

    def ensure_state(self, p, group=None):
        """The state of `p`, created on first use: a host int `step` and zeroed buffers.  (Also completes a state that came
        from a torch checkpoint without a count or before its first step.)"""
        st = self.state[p]
        if 'step' not in st:
            st['step'] = 0
        for k in self._buffers(group if group is not None else self._group(p)):
            if st.get(k) is None:
                st[k] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def plan_key(self, p, group=None):
        """Everything but `lr` and the step count that a recorded launch of `p` has baked in."""
        g = group if group is not None else self._group(p)
        st = self.ensure_state(p, g)
        return (type(self).__name__, self._hyper(g), self.grad_scale, tuple(st[k].data_ptr() for k in self._buffers(g)))

    def state_tensors(self, p):
        """The state buffers a recorded launch of `p` points into (a plan keeps them alive)."""
        return [self.state[p][k] for k in self._buffers(self._group(p))]

    def advance(self, p):
        """Count a step whose launch somebody else issues (a replayed plan); returns the new 1-based count."""
        st = self.state[p]
        st['step'] += 1
        return st['step']

    def launch(self, p, grad, stream=None, slots=False, group=None):
        """One optimizer step of `p` from the contiguous fp32 device gradient `grad`, enqueued on `stream` (None: torch's current
        stream).  slots: name `lr` and the step count as plan slots (only looked at while a step is being recorded)."""
        if not p.is_cuda or p.dtype != torch.float32 or p.numel() % 4 or not p.is_contiguous():
            raise RuntimeError(f'{type(self).__name__} runs on the HIP path only: contiguous fp32 device parameters with a '
                               'multiple of 4 elements (the model\'s flat parameter)')
        group = group if group is not None else self._group(p)
        stream = N.stream() if stream is None else stream
        st = self.ensure_state(p, group)
        st['step'] += 1                               # a host int (load_state_dict normalises a tensor step)
        N.call('t3d_set_grad_watch', N.ptr(self.watch_word(p.device)))
        try:
            self._call(p, grad, st, group, stream, slots)
        finally:
            N.call('t3d_set_grad_watch', None)            # (process-wide pointer: never left pointing at this optimizer's word)
        torch.autograd.graph.increment_version(p)     # written through a raw pointer: tell version-tracking users

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            for p in group['params']:
                if p.grad is None:
                    continue
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                self.launch(p, g, group=group)
        return loss

    # `step` is a host int here; torch.optim keeps a float tensor (and none at all in SGD).  Checkpoints travel in torch's form,
    # so that a snapshot written by either optimizer loads into the other (build_optimizer falls back to torch.optim for
    # parameters that are not on the GPU), and a loaded device tensor never costs a sync per step.
    def state_dict(self):
        sd = super().state_dict()
        # (the packed state holds the optimizer's own per-parameter dicts: copy before rewriting `step`)
        sd['state'] = {k: ({**st, 'step': torch.tensor(float(st['step']))} if 'step' in st and not torch.is_tensor(st['step'])
                           else st) for k, st in sd['state'].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():
            if 'step' in st:
                st['step'] = int(st['step'].item()) if torch.is_tensor(st['step']) else int(st['step'])
        for g in self.param_groups:
            self._refuse(g)

    # options of the torch class that no kernel here implements: {name: the only value taken}
    _REFUSED = {}

    def _refuse(self, group):
        for k, v in self._REFUSED.items():
            if group.get(k, v) != v:
                raise ValueError(f'{type(self).__name__} does not implement {k}={group[k]!r} (torch.optim does)')


class FusedAdamW(FusedOptimizer):
    """torch.optim.AdamW (decoupled weight decay, no amsgrad / maximize) as one HIP launch per parameter tensor.
    `grad_scale` multiplies the gradient on load (1/world after a summed all-reduce)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError('invalid AdamW hyper-parameter')
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay), grad_scale)

    def _buffers(self, group):
        return ('exp_avg', 'exp_avg_sq')

    def _hyper(self, group):
        return (tuple(group['betas']), group['eps'], group['weight_decay'])

    def _call(self, p, grad, st, group, stream, slots):
        b1, b2 = group['betas']
        N.call('t3d_adamw_step', N.ptr(p), N.ptr(grad), N.ptr(st['exp_avg']), N.ptr(st['exp_avg_sq']), p.numel(),
               float(group['lr']), float(b1), float(b2), float(group['eps']), float(group['weight_decay']), st['step'],
               float(self.grad_scale), stream, slots={5: N.SLOT_LR, 10: N.SLOT_STEP} if slots else None)


class FusedSGD(FusedOptimizer):
    """torch.optim.SGD (momentum, Nesterov, coupled weight decay; dampening 0) as one HIP launch per parameter tensor
    (`t3d_sgd_step`).  State in torch's layout: `momentum_buffer` (none with momentum 0), plus a `step` count that torch does
    not keep -- the divergence watch reports steps by it.  torch.optim.SGD ignores the extra entry of a snapshot written here,
    and a torch snapshot without one resumes here counting from 0."""
    _REFUSED = dict(dampening=0, maximize=False)

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 grad_scale=1.0):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError('invalid SGD hyper-parameter')
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        d = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=maximize)
        self._refuse(d)
        super().__init__(params, d, grad_scale)

    def _buffers(self, group):
        return ('momentum_buffer',) if group['momentum'] != 0 else ()

    def _hyper(self, group):
        return (group['momentum'], group['weight_decay'], bool(group['nesterov']))

    def _call(self, p, grad, st, group, stream, slots):
        if group['nesterov'] and group['momentum'] <= 0:
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        N.call('t3d_sgd_step', N.ptr(p), N.ptr(grad), N.ptr(st.get('momentum_buffer') if group['momentum'] != 0 else None),
               p.numel(), float(group['lr']), float(group['momentum']), float(group['weight_decay']), int(bool(group['nesterov'])),
               st['step'], float(self.grad_scale), stream, slots={4: N.SLOT_LR, 8: N.SLOT_STEP} if slots else None)


class FusedRMSprop(FusedOptimizer):
    """torch.optim.RMSprop (not centered, no momentum) as one HIP launch per parameter tensor (`t3d_rmsprop_step`); state
    `step`, `square_avg`."""
    _REFUSED = dict(momentum=0, centered=False, maximize=False)

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, *, maximize=False,
                 grad_scale=1.0):
        if lr < 0 or eps < 0 or alpha < 0 or weight_decay < 0:
            raise ValueError('invalid RMSprop hyper-parameter')
        d = dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum, centered=centered, maximize=maximize)
        self._refuse(d)
        super().__init__(params, d, grad_scale)

    def _buffers(self, group):
        return ('square_avg',)

    def _hyper(self, group):
        return (group['alpha'], group['eps'], group['weight_decay'])

    def _call(self, p, grad, st, group, stream, slots):
        N.call('t3d_rmsprop_step', N.ptr(p), N.ptr(grad), N.ptr(st['square_avg']), p.numel(), float(group['lr']),
               float(group['alpha']), float(group['eps']), float(group['weight_decay']), st['step'], float(self.grad_scale),
               stream, slots={4: N.SLOT_LR, 8: N.SLOT_STEP} if slots else None)


class FusedAdadelta(FusedOptimizer):
    """torch.optim.Adadelta as one HIP launch per parameter tensor (`t3d_adadelta_step`); state `step`, `square_avg`,
    `acc_delta`."""
    _REFUSED = dict(maximize=False)

    def __init__(self, params, lr=1.0, rho=0.9, eps=1e-6, weight_decay=0, *, maximize=False, grad_scale=1.0):
        if lr < 0 or eps < 0 or not 0 <= rho <= 1 or weight_decay < 0:
            raise ValueError('invalid Adadelta hyper-parameter')
        d = dict(lr=lr, rho=rho, eps=eps, weight_decay=weight_decay, maximize=maximize)
        self._refuse(d)
        super().__init__(params, d, grad_scale)

    def _buffers(self, group):
        return ('square_avg', 'acc_delta')

    def _hyper(self, group):
        return (group['rho'], group['eps'], group['weight_decay'])

    def _call(self, p, grad, st, group, stream, slots):
        N.call('t3d_adadelta_step', N.ptr(p), N.ptr(grad), N.ptr(st['square_avg']), N.ptr(st['acc_delta']), p.numel(),
               float(group['lr']), float(group['rho']), float(group['eps']), float(group['weight_decay']), st['step'],
               float(self.grad_scale), stream, slots={5: N.SLOT_LR, 9: N.SLOT_STEP} if slots else None)


def build_optimizer(cfg, net):
    assert cfg.optim.name in AVAILABLE_OPTIMS
    params = list(net.parameters())
    o = cfg.optim
    fused = all(p.is_cuda for p in params)        # otherwise the torch class, for parameters that are not on the GPU
    if o.name == 'adadelta':
        return (FusedAdadelta if fused else torch.optim.Adadelta)(params, lr=o.lr, rho=o.rho, weight_decay=o.wd)
    if o.name == 'adam':
        return (FusedAdamW if fused else torch.optim.AdamW)(params, lr=o.lr, betas=tuple(o.betas), weight_decay=o.wd)
    if o.name == 'rmsprop':
        return (FusedRMSprop if fused else torch.optim.RMSprop)(params, lr=o.lr, weight_decay=o.wd, alpha=o.alpha)
    return (FusedSGD if fused else torch.optim.SGD)(params, lr=o.lr, weight_decay=o.wd, momentum=o.momentum, nesterov=o.nesterov)
