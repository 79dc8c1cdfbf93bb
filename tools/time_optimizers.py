"""Cost of the four optimizer names on one GPU: the kernel optimizers of builders/optim_builder.py (csrc/misc.hip) against
the framework optimizers they replace.

  1. Kernels alone: HIP-event time of one `t3d_adamw_step` / `t3d_sgd_step` / `t3d_rmsprop_step` / `t3d_adadelta_step` launch
     over the flat parameter sizes of MobileNetV2 and MobileNetV3-large, the four alternated launch by launch in one loop;
     median / min microseconds and algorithmic bytes / time (20 B per parameter for SGD and RMSprop, 28 B for Adadelta
     and AdamW).
  2. Step time: MobileNetV2, 224x224, B = 256, bf16 storage, through `build_model` / `build_optimizer` /
     `Trainer.train_step`, for each name
       (a) the framework optimizer (a hand-built torch.optim object): the eager form of the step through autograd;
       (b) the kernel optimizer `build_optimizer` returns: the recorded step plan, one `t3d_plan_run` per step,
     all eight alternated block by block in the same process (`--repeats` blocks of `--steps` steps each, after a warm-up
     that includes the plan's recording).  ms/step is wall time over a block closed by a device synchronisation; host
     ms/step is the time the Python loop needs to issue a short block of 6 steps into an empty queue.
Prints one JSON line per measurement.  Usage: python tools/time_optimizers.py [--steps 30] [--repeats 5] [--batch 256] [--skip-steps]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-object-detection.pytorch_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

NAMES = ('adam', 'sgd', 'rmsprop', 'adadelta')


def flat_sizes():
    from test_host_logic import _cfg
    from torchdet3d.builders import build_model
    return {name: build_model(_cfg(name)).flat.numel() for name in ('mobilenetv2', 'mobilenetv3_large')}


def kernel_times(model, n, reps=60):
    from torchdet3d import _native as N
    g = torch.Generator(device='cuda').manual_seed(0)
    p, gr = torch.randn(n, device='cuda', generator=g), torch.randn(n, device='cuda', generator=g)
    bufs = [torch.zeros(n, device='cuda') for _ in range(2)]
    P = N.ptr
    calls = {        # name -> (arguments without the stream, bytes per parameter); lr 0: the buffers stay finite over any number of launches
        't3d_adamw_step': ((P(p), P(gr), P(bufs[0]), P(bufs[1]), n, 0.0, 0.9, 0.999, 1e-8, 1e-4, 1, 1.0), 28),
        't3d_sgd_step': ((P(p), P(gr), P(bufs[0]), n, 0.0, 0.9, 1e-4, 1, 1, 1.0), 20),
        't3d_rmsprop_step': ((P(p), P(gr), P(bufs[0]), n, 0.0, 0.99, 1e-8, 1e-4, 1, 1.0), 20),
        't3d_adadelta_step': ((P(p), P(gr), P(bufs[0]), P(bufs[1]), n, 0.0, 0.9, 1e-6, 1e-4, 1, 1.0), 28),
    }
    st = N.stream()
    for _ in range(5):
        for name, (args, _) in calls.items():
            N.call(name, *args, st)
    ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for name in calls}
    for r in range(reps):
        for name, (args, _) in calls.items():
            e0, e1 = ev[name][r]
            e0.record()
            N.call(name, *args, st)
            e1.record()
    torch.cuda.synchronize()
    out = []
    for name, (_, bpp) in calls.items():
        t = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev[name])
        med = t[len(t) // 2]
        out.append(dict(what='kernel', entry=name, model=model, n=n, MB=round(n * bpp / 1e6, 1), median_us=round(med, 2), min_us=round(t[0], 2),
                        p90_us=round(t[int(len(t) * 0.9)], 2), GBps_median=round(n * bpp / med / 1e3, 1), GBps_best=round(n * bpp / t[0] / 1e3, 1)))
    return out


def framework_optimizer(cfg, model):
    """What build_optimizer returned before the kernel optimizers existed for `cfg.optim.name`."""
    o, ps = cfg.optim, list(model.parameters())
    if o.name == 'adadelta':
        return torch.optim.Adadelta(ps, lr=o.lr, rho=o.rho, weight_decay=o.wd)
    if o.name == 'adam':
        return torch.optim.AdamW(ps, lr=o.lr, betas=tuple(o.betas), weight_decay=o.wd)
    if o.name == 'rmsprop':
        return torch.optim.RMSprop(ps, lr=o.lr, weight_decay=o.wd, alpha=o.alpha)
    return torch.optim.SGD(ps, lr=o.lr, weight_decay=o.wd, momentum=o.momentum, nesterov=o.nesterov)


def make_trainer(name, form, batches, warm=6):
    from test_host_logic import _cfg
    from torchdet3d.builders import build_loss, build_model, build_optimizer
    from torchdet3d.losses import LossManager
    from torchdet3d.trainer import Trainer
    cfg = _cfg('mobilenetv2')
    cfg.model.storage_dtype, cfg.model.eval_storage_dtype, cfg.optim.name = 'bf16', None, name
    torch.manual_seed(3)
    model = build_model(cfg).to('cuda')
    model.net.reset_parameters(seed=3)
    opt = framework_optimizer(cfg, model) if form == 'framework_eager' else build_optimizer(cfg, model)
    lm = LossManager(build_loss(cfg), cfg.loss.coeffs, cfg.loss.alwa)
    tr = Trainer(model, None, opt, None, lm, None, 1, '', device='cuda', save_chkpt=False)
    model.train()
    for i in range(warm):                 # (two direct steps, the recording, replays)
        tr.train_step(*batches[i % 3], i)
    torch.cuda.synchronize()
    return tr


def step_times(B, steps, repeats, host_steps=6):
    """Every (name, form) pair is built first; a repeat then runs one block of each, so that all eight see the same drift of
    the clocks.  The host figure comes from short blocks of their own (`host_steps` steps issued into an empty queue: the
    runtime never makes the host wait for queue space)."""
    g = torch.Generator(device='cuda').manual_seed(1)
    batches = [(torch.randn(B, 3, 224, 224, device='cuda', generator=g), torch.rand(B, 9, 2, device='cuda', generator=g),
                torch.randint(0, 9, (B,), device='cuda', generator=g)) for _ in range(3)]
    trainers = {(name, form): make_trainer(name, form, batches) for name in NAMES for form in ('framework_eager', 'kernel_replay')}

    def block(tr, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            tr.train_step(*batches[i % 3], i)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (t2 - t0) * 1e3 / n, (t1 - t0) * 1e3 / n

    ms, host = {k: [] for k in trainers}, {k: [] for k in trainers}
    for _ in range(repeats):
        for k, tr in trainers.items():
            ms[k].append(block(tr, steps)[0])
        for k, tr in trainers.items():
            host[k].append(block(tr, host_steps)[1])
    out = []
    for (name, form), tr in trainers.items():
        k, sp = (name, form), tr._sp
        out.append(dict(what='step', optim=name, form=form, optimizer=type(tr.optimizer).__name__, B=B, steps=steps,
                        replays=sp.replays if sp is not None else 0,
                        ms_per_step=[round(v, 3) for v in ms[k]], ms_median=round(statistics.median(ms[k]), 3),
                        ms_spread=round(max(ms[k]) - min(ms[k]), 3), host_ms_per_step=[round(v, 3) for v in host[k]],
                        host_ms_median=round(statistics.median(host[k]), 3),
                        crops_per_s=round(B * 1e3 / statistics.median(ms[k]), 1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--skip-steps', action='store_true')
    a = ap.parse_args()
    for model, n in flat_sizes().items():
        for r in kernel_times(model, n):
            print(json.dumps(r), flush=True)
    if not a.skip_steps:
        for r in step_times(a.batch, a.steps, a.repeats):
            print(json.dumps(r), flush=True)


if __name__ == '__main__':
    main()
