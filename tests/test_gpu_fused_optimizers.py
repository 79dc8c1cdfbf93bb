"""The kernel optimizers behind the names 'sgd', 'rmsprop' and 'adadelta' (csrc/misc.hip: t3d_sgd_step, t3d_rmsprop_step,
t3d_adadelta_step; builders/optim_builder.py: FusedSGD, FusedRMSprop, FusedAdadelta) against torch.optim, the reference's
implementation (torchdet3d/builders/optim_builder.py:3-19), and inside the step plan (trainer/step_plan.py): the three forms
of the train iteration stay bit-identical under every optimizer name."""
import copy
import struct

import numpy as np
import pytest
import torch

from test_host_logic import _cfg

pytestmark = pytest.mark.gpu

N_ELEMS = 40004


def _classes(name):
    from torchdet3d.builders import optim_builder as OB
    return {'sgd': (OB.FusedSGD, torch.optim.SGD), 'rmsprop': (OB.FusedRMSprop, torch.optim.RMSprop),
            'adadelta': (OB.FusedAdadelta, torch.optim.Adadelta), 'adam': (OB.FusedAdamW, torch.optim.AdamW)}[name]


def _buffers(opt, p):
    """{state name: tensor} of a parameter, without the step count."""
    return {k: v for k, v in opt.state[p].items() if k != 'step' and torch.is_tensor(v)}


def _ulp(x):
    """Spacing of fp32 at the largest magnitude of the (fp64) tensor."""
    return float(np.spacing(np.float32(x.abs().max().item())))


def _within(what, fused, t32, t64, ratios):
    """The bound of the issue: max |fused - fp64| <= 2 * max |torch_fp32 - fp64| + 1 ulp of the largest entry."""
    ef = (fused.double() - t64).abs().max().item()
    et = (t32.double() - t64).abs().max().item()
    ulp = _ulp(t64)
    ratios.setdefault(what.split('@')[0], []).append(ef / et if et > 0 else (0.0 if ef == 0 else float('inf')))
    print(f'{what}: fused-fp64 {ef:.3e}  torch32-fp64 {et:.3e}  ulp {ulp:.3e}  ratio {ef / et if et > 0 else float("nan"):.3f}')
    assert ef <= 2 * et + ulp, f'{what}: fused error {ef:.3e} against fp64, torch fp32 {et:.3e}, ulp {ulp:.3e}'


PARITY = [('sgd', dict(lr=1e-3, momentum=0.9, nesterov=True)), ('sgd', dict(lr=1e-3, momentum=0.9)), ('sgd', dict(lr=1e-3, momentum=0)),
          ('rmsprop', dict(lr=1e-3, alpha=0.99)), ('adadelta', dict(lr=1.0, rho=0.9)), ('adadelta', dict(lr=1e-3, rho=0.9))]


@pytest.mark.parametrize('wd', [1e-4, 0.0])
@pytest.mark.parametrize('name,hyper', PARITY, ids=['sgd-nesterov', 'sgd-momentum', 'sgd-plain', 'rmsprop', 'adadelta-lr1', 'adadelta-lr1e-3'])
def test_kernel_matches_torch_optim_within_twice_its_own_fp32_error(name, hyper, wd):
    """n = 40004, 12 steps, gradients randn * (1 + it), StepLR(3, 0.5) on every side.  The yardstick is torch.optim on the
    device: once in fp32 and once on an fp64 copy of the same data.  After every step, for the parameter and every state
    tensor: max |fused - fp64| <= 2 * max |torch_fp32 - fp64| + 1 ulp (fp32) of the largest entry -- both are correctly
    ordered fp32 evaluations of the same formulas that differ in fma contraction and in the rounding of sqrt / divide, so
    neither should be further from the exact result than twice the other.

    Observed on an MI355X (largest ratio fused error / torch fp32 error over the 12 steps; 0/0 counted as 0):
    sgd (Nesterov, momentum, plain; both weight decays): parameter 1.00, momentum_buffer 1.00;
    rmsprop: parameter 1.00, square_avg 1.51 (wd 1e-4) / 1.34 (wd 0);
    adadelta lr 1.0: parameter 1.00, square_avg 1.39 / 1.45, acc_delta 1.48 / 1.55;
    adadelta lr 1e-3: parameter 1.00, square_avg 1.45 / 1.45, acc_delta 1.49 / 1.55.
    The errors themselves after 12 steps, for torch's fp32 run and for the kernel alike: parameters 7e-7 .. 1.1e-6 (about
    2 ulp of the largest), square_avg about 1 ulp of its largest entry (4e-6 under rmsprop, 3e-5 under adadelta), acc_delta
    5e-11 (about 4 ulp).
    """
    fused_cls, torch_cls = _classes(name)
    g = torch.Generator().manual_seed(0)
    p0 = torch.randn(N_ELEMS, generator=g)
    pa = torch.nn.Parameter(p0.clone().cuda())
    pb = torch.nn.Parameter(p0.clone().cuda())
    pc = torch.nn.Parameter(p0.double().cuda())
    oa, ob, oc = fused_cls([pa], weight_decay=wd, **hyper), torch_cls([pb], weight_decay=wd, **hyper), torch_cls([pc], weight_decay=wd, **hyper)
    scheds = [torch.optim.lr_scheduler.StepLR(o, 3, 0.5) for o in (oa, ob, oc)]
    ratios = {}
    for it in range(12):
        gr = (torch.randn(N_ELEMS, generator=g) * (1 + it)).cuda()
        pa.grad, pb.grad, pc.grad = gr.clone(), gr.clone(), gr.double()
        v0 = pa._version
        for o in (oa, ob, oc):
            o.step()
        assert pa._version > v0                                    # version-tracking users (engine._pack) see the update
        for s in scheds:
            s.step()
        _within(f'param@{it}', pa.detach(), pb.detach(), pc.detach(), ratios)
        sa, sb, sc = _buffers(oa, pa), _buffers(ob, pb), _buffers(oc, pc)
        assert set(sa) == set(sb) == set(sc), (set(sa), set(sb))
        for k in sb:
            _within(f'{k}@{it}', sa[k], sb[k], sc[k], ratios)
    print('RATIOS', name, hyper, wd, {k: round(max(v), 3) for k, v in ratios.items()})
    assert oa.state[pa]['step'] == 12 and oa.first_nonfinite_step() is None


@pytest.mark.parametrize('name,hyper', [('sgd', dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-4)),
                                        ('sgd', dict(lr=1e-2, momentum=0, weight_decay=1e-4)),
                                        ('rmsprop', dict(lr=1e-3, alpha=0.99, weight_decay=1e-4)),
                                        ('adadelta', dict(lr=1.0, rho=0.9, weight_decay=1e-4))],
                         ids=['sgd-nesterov', 'sgd-plain', 'rmsprop', 'adadelta'])
@pytest.mark.parametrize('src', ['torch', 'fused'])
def test_checkpoints_cross_between_the_kernel_and_the_torch_optimizer(name, hyper, src):
    """A snapshot written by either class loads into the other (and into torch.optim on an fp64 copy, the yardstick); one
    more step on each side agrees within the bound of the parity test.  The saved `step` entries are tensors."""
    fused_cls, torch_cls = _classes(name)
    g = torch.Generator().manual_seed(1)
    p0 = torch.randn(N_ELEMS, generator=g)
    ps = torch.nn.Parameter(p0.clone().cuda())
    osrc = (torch_cls if src == 'torch' else fused_cls)([ps], **hyper)
    for it in range(3):
        ps.grad = (torch.randn(N_ELEMS, generator=g) * (1 + it)).cuda()
        osrc.step()
    sd = osrc.state_dict()
    for st in sd['state'].values():
        assert 'step' not in st or torch.is_tensor(st['step'])
    if src == 'fused':
        assert torch.is_tensor(sd['state'][0]['step']) and float(sd['state'][0]['step']) == 3.0
    pa = torch.nn.Parameter(ps.detach().clone())
    pb = torch.nn.Parameter(ps.detach().clone())
    pc = torch.nn.Parameter(ps.detach().double())
    oa, ob, oc = fused_cls([pa], **hyper), torch_cls([pb], **hyper), torch_cls([pc], **hyper)
    for o in (oa, ob, oc):
        o.load_state_dict(copy.deepcopy(sd))
    # (torch.optim.SGD keeps no count: a snapshot of it resumes counting from 0)
    assert oa.state[pa].get('step', 0) == (0 if (src == 'torch' and name == 'sgd') else 3)
    gr = (torch.randn(N_ELEMS, generator=g) * 4).cuda()
    pa.grad, pb.grad, pc.grad = gr.clone(), gr.clone(), gr.double()
    for o in (oa, ob, oc):
        o.step()
    ratios = {}
    _within('param', pa.detach(), pb.detach(), pc.detach(), ratios)
    sa, sb, sc = _buffers(oa, pa), _buffers(ob, pb), _buffers(oc, pc)
    assert set(sa) == set(sb)
    for k in sb:
        _within(k, sa[k], sb[k], sc[k], ratios)
    assert torch.is_tensor(oa.state_dict()['state'][0]['step'])
    assert int(oa.state_dict()['state'][0]['step']) == oa.state[pa]['step']


def test_builder_returns_the_kernel_optimizer_for_every_name_on_a_device_model():
    from torchdet3d.builders import build_model, build_optimizer
    from torchdet3d.trainer.step_plan import StepPlan
    from torchdet3d.builders import build_loss
    from torchdet3d.losses import LossManager
    cfg = _cfg('mobilenetv2')
    model = build_model(cfg).to('cuda')
    lm = LossManager(build_loss(cfg), cfg.loss.coeffs, cfg.loss.alwa)
    for name in ('sgd', 'rmsprop', 'adam', 'adadelta'):
        cfg.optim.name = name
        opt = build_optimizer(cfg, model)
        fused_cls, torch_cls = _classes(name)
        assert type(opt) is fused_cls and not isinstance(opt, torch_cls)
        assert StepPlan.usable(model, lm, opt)
        g = opt.param_groups[0]
        assert g['lr'] == cfg.optim.lr and g['weight_decay'] == cfg.optim.wd
    cfg.optim.name = 'sgd'
    g = build_optimizer(cfg, model).param_groups[0]
    assert g['momentum'] == 0.9 and g['nesterov'] is True
    assert not StepPlan.usable(model, lm, torch.optim.RMSprop(model.parameters(), lr=0.1))


def test_options_the_kernels_do_not_implement_are_refused_and_bad_parameters_fail_loudly():
    from torchdet3d.builders.optim_builder import FusedAdadelta, FusedRMSprop, FusedSGD
    p = torch.nn.Parameter(torch.zeros(8, device='cuda'))
    for make in (lambda: FusedSGD([p], dampening=0.1, momentum=0.9), lambda: FusedSGD([p], maximize=True),
                 lambda: FusedSGD([p], nesterov=True), lambda: FusedRMSprop([p], centered=True),
                 lambda: FusedRMSprop([p], momentum=0.9), lambda: FusedRMSprop([p], maximize=True),
                 lambda: FusedAdadelta([p], maximize=True), lambda: FusedAdadelta([p], rho=1.5)):
        with pytest.raises(ValueError):
            make()
    # a torch snapshot that carries such an option is refused on load, not silently stepped without it
    t = torch.optim.RMSprop([torch.nn.Parameter(torch.zeros(8, device='cuda'))], centered=True)
    with pytest.raises(ValueError):
        FusedRMSprop([p]).load_state_dict(t.state_dict())
    for cls in (FusedSGD, FusedRMSprop, FusedAdadelta):
        for bad in (torch.zeros(6, device='cuda'), torch.zeros(8, device='cuda', dtype=torch.float64), torch.zeros(8)):
            q = torch.nn.Parameter(bad)
            q.grad = torch.ones_like(q)
            with pytest.raises(RuntimeError, match='HIP path only'):
                cls([q]).step()


def test_entry_points_check_their_arguments():
    from torchdet3d import _native as N
    lib = N.lib()
    x = torch.zeros(16, device='cuda')
    a, st = x.data_ptr(), N.stream()
    assert lib.t3d_sgd_step(None, a, a, 16, 0.1, 0.9, 0.0, 0, 1, 1.0, st) == -1
    assert lib.t3d_sgd_step(a, a, None, 16, 0.1, 0.9, 0.0, 0, 1, 1.0, st) == -1          # a momentum without its buffer
    assert lib.t3d_sgd_step(a, a, None, 16, 0.1, 0.0, 0.0, 1, 1, 1.0, st) == -1          # Nesterov without a momentum
    assert lib.t3d_sgd_step(a, a, a, 18, 0.1, 0.9, 0.0, 0, 1, 1.0, st) == -1
    assert lib.t3d_sgd_step(a, a, a, 16, 0.1, 0.9, 0.0, 0, 0, 1.0, st) == -1
    assert lib.t3d_rmsprop_step(a, a, None, 16, 0.1, 0.99, 1e-8, 0.0, 1, 1.0, st) == -1
    assert lib.t3d_rmsprop_step(a, a, a, 0, 0.1, 0.99, 1e-8, 0.0, 1, 1.0, st) == -1
    assert lib.t3d_rmsprop_step(a, a, a, 16, 0.1, 0.99, 1e-8, 0.0, 0, 1.0, st) == -1
    assert lib.t3d_adadelta_step(a, a, a, None, 16, 1.0, 0.9, 1e-6, 0.0, 1, 1.0, st) == -1
    assert lib.t3d_adadelta_step(a, a, a, a, 14, 1.0, 0.9, 1e-6, 0.0, 1, 1.0, st) == -1
    assert lib.t3d_adadelta_step(a, a, a, a, 16, 1.0, 0.9, 1e-6, 0.0, -1, 1.0, st) == -1
    torch.cuda.synchronize()
    assert torch.equal(x, torch.zeros_like(x))                                           # nothing was launched


# ---- the step plan under every optimizer name (the harness of tests/test_gpu_step_plan.py with cfg.optim.name set) --------------
def _objects(name, dtype, optim, nc=9, seed=3):
    from torchdet3d.builders import build_loss, build_model, build_optimizer
    from torchdet3d.losses import LossManager
    from torchdet3d.trainer import Trainer
    cfg = _cfg(name, nc=nc)
    cfg.model.storage_dtype = dtype
    cfg.model.eval_storage_dtype = None
    cfg.optim.name = optim
    torch.manual_seed(seed)
    model = build_model(cfg).to('cuda')
    model.net.reset_parameters(seed=seed)
    opt = build_optimizer(cfg, model)
    lm = LossManager(build_loss(cfg), cfg.loss.coeffs, cfg.loss.alwa)
    tr = Trainer(model, None, opt, None, lm, None, 1, '', device='cuda', save_chkpt=False)
    model.train()
    return model, opt, lm, tr


def _batches(B, S, nb=3, seed=11, nc=9):
    g = torch.Generator(device='cuda').manual_seed(seed)
    imgs = [torch.randn(B, 3, S, S, device='cuda', generator=g) for _ in range(nb)]
    gts = [torch.rand(B, 9, 2, device='cuda', generator=g) for _ in range(nb)]
    cats = [torch.randint(0, nc, (B,), device='cuda', generator=g) for _ in range(nb)]
    return imgs, gts, cats


def _bits(r):
    """A metric dict as bit patterns (equal NaNs compare equal)."""
    return {k: struct.pack('<d', float(v)) for k, v in dict(r).items()}


def _run(name, dtype, optim, B, S, steps, mode, lr_at=None):
    """mode: 'eager' | 'direct' | 'replay'.  Returns (weights, buffers, optimizer state, per-step metric dicts, Trainer)."""
    from torchdet3d.trainer import step_plan
    model, opt, lm, tr = _objects(name, dtype, optim)
    assert type(opt) is _classes(optim)[0]
    imgs, gts, cats = _batches(B, S)
    assert tr._step_plan() is not None, 'the kernel optimizer must be admitted to the step plan'
    if mode == 'eager':
        tr._sp = None
    old = step_plan.REPLAY
    step_plan.REPLAY = mode == 'replay'
    try:
        res = []
        for i in range(steps):
            if lr_at is not None and i == lr_at:
                opt.param_groups[0]['lr'] = 3e-4           # what an LR scheduler does between two iterations
            j = i % len(imgs)
            res.append(_bits(tr.train_step(imgs[j], gts[j], cats[j], i)))
    finally:
        step_plan.REPLAY = old
    torch.cuda.synchronize()
    st = opt.state[model.flat]
    return (model.net.flat.clone(), {k: v.clone() for k, v in model.net.buffers.items()},
            (st['step'], {k: v.clone() for k, v in _buffers(opt, model.flat).items()}), res, tr)


def _same(a, b):
    wa, ba, oa, ra, _ = a
    wb, bb, ob, rb, _ = b
    assert torch.equal(wa, wb), f'weights differ: max {(wa - wb).abs().max().item():.3e}'
    for k in ba:
        assert torch.equal(ba[k], bb[k]), k
    assert oa[0] == ob[0] and set(oa[1]) == set(ob[1])
    for k in oa[1]:
        assert torch.equal(oa[1][k], ob[1][k]), k
    assert ra == rb, (ra[-1], rb[-1])


@pytest.mark.parametrize('optim', ['sgd', 'rmsprop', 'adadelta'])
@pytest.mark.parametrize('name,dtype,B,S', [('mobilenetv2', 'bf16', 16, 96), ('mobilenetv3_small', 'bf16', 8, 96), ('mobilenetv2', 'f32', 8, 96)])
def test_three_forms_of_the_step_are_bit_identical_under_every_optimizer(name, dtype, B, S, optim):
    steps = 7
    eager = _run(name, dtype, optim, B, S, steps, 'eager', lr_at=5)
    direct = _run(name, dtype, optim, B, S, steps, 'direct', lr_at=5)
    replay = _run(name, dtype, optim, B, S, steps, 'replay', lr_at=5)
    _same(eager, direct)
    _same(eager, replay)
    expected = {'sgd': {'momentum_buffer'}, 'rmsprop': {'square_avg'}, 'adadelta': {'square_avg', 'acc_delta'}}[optim]
    assert set(replay[2][1]) == expected and replay[2][0] == steps
    sp = replay[4]._sp
    assert sp is not None and sp.rec is not None and sp.replays == steps - 3      # two warm steps, one recorded, the rest replayed
    assert direct[4]._sp.replays == 0 and eager[4]._sp is None
    entry = {'sgd': 't3d_sgd_step', 'rmsprop': 't3d_rmsprop_step', 'adadelta': 't3d_adadelta_step'}[optim]
    assert [c[0] for c in sp.rec.calls].count(entry) == 1                         # the optimizer launch is inside the plan


@pytest.mark.parametrize('optim,knob,value', [('sgd', 'momentum', 0.8), ('rmsprop', 'alpha', 0.9), ('adadelta', 'rho', 0.95)])
def test_a_hyper_parameter_change_rerecords_and_a_learning_rate_change_does_not(optim, knob, value):
    from torchdet3d.trainer import step_plan
    assert step_plan.REPLAY
    model, opt, lm, tr = _objects('mobilenetv2', 'bf16', optim)
    model2, opt2, lm2, tr2 = _objects('mobilenetv2', 'bf16', optim)
    tr2._sp = None                                                        # the eager twin
    imgs, gts, cats = _batches(8, 96)
    replays = []
    for i in range(13):
        if i == 5:
            opt.param_groups[0][knob] = opt2.param_groups[0][knob] = value
        if i == 10:
            opt.param_groups[0]['lr'] = opt2.param_groups[0]['lr'] = 2.5e-4
        j = i % 3
        r1, r2 = _bits(tr.train_step(imgs[j], gts[j], cats[j], i)), _bits(tr2.train_step(imgs[j], gts[j], cats[j], i))
        assert r1 == r2, (i, r1, r2)
        replays.append(tr._sp.replays)
    torch.cuda.synchronize()
    assert torch.equal(model.net.flat, model2.net.flat)
    for k, v in _buffers(opt, model.flat).items():
        assert torch.equal(v, opt2.state[model2.flat][k]), k
    # steps 0-1 warm, 2 recorded, 3-4 replayed; the new hyper-parameter costs two warm steps and a recording (5-7), 8-9
    # replayed; the new learning rate costs nothing (10-12 replayed)
    assert replays == [0, 0, 0, 1, 2, 2, 2, 2, 3, 4, 5, 6, 7], replays


@pytest.mark.parametrize('name,hyper', [('sgd', dict(lr=1e-2, momentum=0.9, nesterov=True)), ('sgd', dict(lr=1e-2)),
                                        ('rmsprop', dict(lr=1e-3)), ('adadelta', dict(lr=1.0))],
                         ids=['sgd-nesterov', 'sgd-plain', 'rmsprop', 'adadelta'])
def test_divergence_watch_names_the_first_step_with_a_non_finite_gradient(name, hyper):
    fused_cls, _ = _classes(name)
    g = torch.Generator().manual_seed(2)
    p = torch.nn.Parameter(torch.randn(4096, generator=g).cuda())
    opt = fused_cls([p], **hyper)
    assert opt.first_nonfinite_step() is None
    k = 4
    for it in range(1, 7):
        gr = torch.randn(4096, generator=g).cuda()
        if it == k:
            gr[1234] = float('inf')
        if it == k + 1:
            gr[7] = float('nan')
        p.grad = gr
        opt.step()
        assert opt.first_nonfinite_step() == (None if it < k else k), it
    assert opt.state[p]['step'] == 6


@pytest.mark.parametrize('name,hyper', [('sgd', dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-4)),
                                        ('sgd', dict(lr=1e-2, momentum=0, weight_decay=1e-4)),
                                        ('rmsprop', dict(lr=1e-3, weight_decay=1e-4)), ('adadelta', dict(lr=1.0, weight_decay=1e-4))],
                         ids=['sgd-nesterov', 'sgd-plain', 'rmsprop', 'adadelta'])
def test_grad_scale_of_a_power_of_two_is_exact(name, hyper):
    """grad_scale = 0.5 on g equals grad_scale = 1 on 0.5 * g bit for bit."""
    fused_cls, _ = _classes(name)
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(N_ELEMS, generator=g)
    pa, pb = torch.nn.Parameter(p0.clone().cuda()), torch.nn.Parameter(p0.clone().cuda())
    oa, ob = fused_cls([pa], grad_scale=0.5, **hyper), fused_cls([pb], **hyper)
    for it in range(4):
        gr = (torch.randn(N_ELEMS, generator=g) * (1 + it)).cuda()
        pa.grad, pb.grad = gr.clone(), gr * 0.5
        oa.step()
        ob.step()
        assert torch.equal(pa, pb), it
        for k, v in _buffers(oa, pa).items():
            assert torch.equal(v, ob.state[pb][k]), (k, it)


def test_trainer_reports_nan_from_the_diverging_step_on_under_sgd():
    """`Trainer.train`'s per-step divergence report (trainer/train.py) works through `first_nonfinite_step` of any kernel
    optimizer: the iterations before the one with an inf in its input keep their finite loss."""
    from torchdet3d.trainer import Trainer
    model, opt, lm, _ = _objects('mobilenetv2', 'bf16', 'sgd')
    imgs, gts, cats = _batches(8, 96, nb=6)
    imgs[4] = imgs[4].clone()
    imgs[4][2, 0, 10:14, 10:14] = float('inf')

    class W:
        def __init__(self): self.rows = []
        def add_scalar(self, tag, v, global_step=None):
            if tag == 'Train/loss': self.rows.append((global_step, v))

    w = W()
    tr = Trainer(model, list(zip(imgs, gts, cats)), opt, None, lm, w, 1, '', device='cuda', save_chkpt=False, print_freq=100)
    tr.train(0, False)
    losses = [v for _, v in sorted(w.rows)]
    assert len(losses) == 6
    assert all(v == v for v in losses[:4]), losses
    assert all(v != v for v in losses[4:]), losses
    assert opt.first_nonfinite_step() == 5


def test_a_feature_only_pass_leaves_the_exact_pool_switch_off_for_the_next_model():
    """`Net.extract_features` / `forward_taps` of a model with squeeze-excite blocks used to return with the process-wide
    exact-pool switch (t3d_set_exact_pool) on; the first train forward of the next MobileNetV3-small in the process -- whose
    first block pools AFTER the activation, in floating point -- then differed from every later one, and with it whichever
    form of the step a comparison happened to run first."""
    from torchdet3d.models.engine import Net
    imgs, gts, cats = _batches(8, 96)
    big = Net('mobilenetv3_large', 9, 'cuda', torch.bfloat16)
    big.reset_parameters(seed=1)
    with torch.no_grad():
        big.extract_features(imgs[0])
    del big
    outs = []
    for _ in range(2):
        model, _, _, _ = _objects('mobilenetv3_small', 'bf16', 'sgd')
        kp, _ = model.net.forward(imgs[0], cats[0], train=True)
        outs.append(kp.clone())
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
