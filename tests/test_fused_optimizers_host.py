"""Host side of the kernel optimizers (builders/optim_builder.py: FusedSGD, FusedRMSprop, FusedAdadelta) -- what can be
checked without a GPU: constructor defaults equal torch.optim's, unreachable options are refused, the checkpoint form is
torch's, the C ABI and the plan's entry table know the three entry points, and the yardstick of the GPU parity test
(tests/test_gpu_fused_optimizers.py) is neither vacuous nor zero."""
import copy
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_host_logic import _cfg

PAIRS = [('FusedSGD', torch.optim.SGD), ('FusedRMSprop', torch.optim.RMSprop), ('FusedAdadelta', torch.optim.Adadelta),
         ('FusedAdamW', torch.optim.AdamW)]


def _fused(name):
    from torchdet3d.builders import optim_builder as OB
    return getattr(OB, name)


@pytest.mark.parametrize('name,torch_cls', PAIRS)
def test_constructor_hyper_parameters_and_defaults_are_torchs(name, torch_cls):
    ours = inspect.signature(_fused(name).__init__).parameters
    theirs = inspect.signature(torch_cls.__init__).parameters
    for k, v in ours.items():
        if k in ('self', 'params', 'grad_scale'):
            continue
        assert k in theirs, f'{name}: {k} is not a torch.optim.{torch_cls.__name__} argument'
        assert v.default == theirs[k].default, (name, k, v.default, theirs[k].default)
    p = torch.nn.Parameter(torch.zeros(8))
    a, b = _fused(name)([p]), torch_cls([p])
    for k, v in a.param_groups[0].items():
        if k != 'params':
            assert b.param_groups[0][k] == v, (name, k)
    assert a.grad_scale == 1.0 and a.first_nonfinite_step() is None


def test_unreachable_options_are_refused_not_ignored():
    p = torch.nn.Parameter(torch.zeros(8))
    S, R, A = _fused('FusedSGD'), _fused('FusedRMSprop'), _fused('FusedAdadelta')
    for make in (lambda: S([p], momentum=0.9, dampening=0.5), lambda: S([p], maximize=True), lambda: S([p], nesterov=True),
                 lambda: S([p], lr=-1.0), lambda: R([p], centered=True), lambda: R([p], momentum=0.5), lambda: R([p], maximize=True),
                 lambda: A([p], maximize=True), lambda: A([p], rho=2.0)):
        with pytest.raises(ValueError):
            make()
    with pytest.raises(ValueError):                    # ... and neither does a torch snapshot smuggle one in
        S([p], momentum=0.9).load_state_dict(torch.optim.SGD([p], lr=0.1, momentum=0.9, dampening=0.5).state_dict())


@pytest.mark.parametrize('name,torch_cls', PAIRS[:3])
def test_a_host_parameter_fails_loudly_and_the_builder_keeps_torch_optim_for_it(name, torch_cls):
    from torchdet3d.builders import build_model, build_optimizer
    p = torch.nn.Parameter(torch.zeros(8))
    p.grad = torch.ones(8)
    with pytest.raises(RuntimeError, match='HIP path only'):
        _fused(name)([p]).step()
    cfg = _cfg('mobilenetv2')
    cfg.optim.name = {'FusedSGD': 'sgd', 'FusedRMSprop': 'rmsprop', 'FusedAdadelta': 'adadelta'}[name]
    assert type(build_optimizer(cfg, build_model(cfg))) is torch_cls


@pytest.mark.parametrize('name,torch_cls,kw', [('FusedSGD', torch.optim.SGD, dict(lr=0.1, momentum=0.9, nesterov=True)),
                                               ('FusedRMSprop', torch.optim.RMSprop, dict(lr=0.01)),
                                               ('FusedAdadelta', torch.optim.Adadelta, dict(lr=1.0))])
def test_checkpoint_form_is_torchs_both_ways(name, torch_cls, kw):
    """torch -> kernel optimizer: `step` becomes a host int (0 where torch keeps none) and is saved as a tensor again;
    kernel optimizer -> torch: the loaded optimizer steps (on the CPU) exactly like one that never left torch."""
    g = torch.Generator().manual_seed(0)
    p0 = torch.randn(64, generator=g)
    pt = torch.nn.Parameter(p0.clone())
    t = torch_cls([pt], **kw)
    grads = [torch.randn(64, generator=g) for _ in range(4)]
    for gr in grads[:3]:
        pt.grad = gr.clone()
        t.step()
    pf = torch.nn.Parameter(pt.detach().clone())
    f = _fused(name)([pf], **kw)
    f.load_state_dict(copy.deepcopy(t.state_dict()))      # (load_state_dict keeps the tensors it is handed)
    st = f.state[pf]
    assert all(not torch.is_tensor(v) for k, v in st.items() if k == 'step')
    assert f.ensure_state(pf)['step'] == (0 if name == 'FusedSGD' else 3)
    sd = f.state_dict()
    assert torch.is_tensor(sd['state'][0]['step'])
    assert set(sd['state'][0]) - {'step'} == set(t.state_dict()['state'][0]) - {'step'}
    # back into torch: one more step equals the step of the optimizer that never left
    p2 = torch.nn.Parameter(pt.detach().clone())
    t2 = torch_cls([p2], **kw)
    t2.load_state_dict(copy.deepcopy(sd))
    pt.grad, p2.grad = grads[3].clone(), grads[3].clone()
    t.step()
    t2.step()
    assert torch.equal(pt, p2)


def test_lr_and_step_sit_where_the_optimizers_bind_the_plan_slots():
    """(That the three entry points are declared, typed as declared and recordable: tests/test_abi.py.)"""
    hdr = open(os.path.join(ROOT, 'include', 't3d.h')).read()
    for n in ('t3d_sgd_step', 't3d_rmsprop_step', 't3d_adadelta_step'):
        decl = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % n, hdr).group(1)
        names = [a.split()[-1].lstrip('*') for a in decl.split(',')]
        src = open(os.path.join(ROOT, '3d-object-detection.pytorch_amd', 'torchdet3d', 'builders', 'optim_builder.py')).read()
        m = re.search(r"N\.call\('%s'.*?slots=\{(\d+): N\.SLOT_LR, (\d+): N\.SLOT_STEP\}" % n, src, flags=re.S)
        assert names[int(m.group(1))] == 'lr' and names[int(m.group(2))] == 'step', (n, names)


def _torch_fp32_error(torch_cls, kw, n=40004, steps=12):
    g = torch.Generator().manual_seed(0)
    p0 = torch.randn(n, generator=g)
    pb, pc = torch.nn.Parameter(p0.clone()), torch.nn.Parameter(p0.double())
    ob, oc = torch_cls([pb], **kw), torch_cls([pc], **kw)
    sb, sc = (torch.optim.lr_scheduler.StepLR(o, 3, 0.5) for o in (ob, oc))
    for it in range(steps):
        gr = torch.randn(n, generator=g) * (1 + it)
        pb.grad, pc.grad = gr.clone(), gr.double()
        ob.step(); oc.step(); sb.step(); sc.step()
    err = (pb.detach().double() - pc.detach()).abs().max().item()
    return err, float(np.spacing(np.float32(pc.detach().abs().max().item())))


@pytest.mark.parametrize('torch_cls,kw', [(torch.optim.SGD, dict(lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-4)),
                                          (torch.optim.RMSprop, dict(lr=1e-3, alpha=0.99, weight_decay=1e-4)),
                                          (torch.optim.Adadelta, dict(lr=1.0, rho=0.9, weight_decay=1e-4))])
def test_the_parity_yardstick_is_neither_vacuous_nor_zero(torch_cls, kw):
    """The GPU parity test allows twice torch's own fp32-vs-fp64 error plus one ulp: that error is a few ulp of the largest
    parameter after 12 steps -- not zero, and nowhere near the size of an update."""
    err, ulp = _torch_fp32_error(torch_cls, kw)
    assert 0 < err <= 16 * ulp, (err, ulp)
