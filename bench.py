#!/usr/bin/env python3
"""Headline benchmark: regression-train crops/sec, MobileNetV2 9-class, 224x224 crops, per-GPU batch 256,
bf16 activation storage (fp32 accumulate, fp32 master weights), on N MI355X of one node.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...   (N > 1)

One "step" = one full train iteration of the hot path over one synthetic batch that is already resident
in HBM: forward (train-mode BatchNorm) -> fused losses l1 + 0.1*add_loss + 0.2*cross_entropy and their
gradients -> hand-derived backward -> (N > 1: bucketed RCCL all-reduce overlapped with the backward) ->
AdamW update.  Prints ONE JSON line (rank 0).  A plain run does only what that line's headline needs: set-up, the W
warm-up steps, the K timed steps (with --dump-outputs DIR, then what the last of them computed as DIR/<name>.npy).
With --full, also measured and reported on the same line:
  host_issue_ms_per_step (config) the host time to enqueue one step, from two extra untimed steps ahead of the timed ones
  roofline      the depthwise kernels (the ones the north-star names), each family -- forward / backward x
                stride 1 / 2, by its rocprof kernel name -- timed with HIP events on the launch stream inside
                the timed steps: algorithmic HBM bytes / measured time vs 8 TB/s; the headline entry is the
                family with the most device time (MobileNetV2: the stride-1 backward, `dw3_bwd2_kernel`)
  cpu_baseline  the CPU oracle (oracle/, a torch-CPU restatement pinned to the reference) running the same
                train step on this host's cores, on a bounded sample (rank 0, N == 1 only)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [ROOT, os.path.join(ROOT, '3d-object-detection.pytorch_amd')]

import torch  # noqa: E402

HBM_PEAK = 8.0e12          # B/s, MI355X HBM3E spec (/opt/skills/guides/MI355X_MICROARCH.md)
MNV2_TRAIN_MB_PER_CROP = 80.66   # algorithmic bytes, bf16, fwd + dgrad + wgrad
CONV_KERNELS = ('t3d_dwconv_fwd', 't3d_dwconv_bwd', 't3d_pwconv_fwd', 't3d_pwconv_dgrad', 't3d_pwconv_wgrad',
                't3d_pwconv_dgrad_yfree', 't3d_pwconv_wgrad_yfree', 't3d_pwconv_fwd_mat', 't3d_pwconv_bwd_yfree',
                't3d_pwconv_wgrad_yfree_finish', 't3d_pwconv_yfree_prep', 't3d_pwconv_yfree_prep2', 't3d_pwconv_bwd_yfree_w',
                't3d_expdw_fwd', 't3d_bn_apply_gram', 't3d_gram_bn_finalize', 't3d_bn_apply', 't3d_bn_finalize')
DW_ENTRIES = ('t3d_dwconv_fwd', 't3d_dwconv_bwd')
# every convolution entry point whose main kernel takes a kernel-exact event pair (T3D_LAUNCH_TIMED in csrc): the families of
# roofline.families (the driver line shows the WORST family beside the north-star's depthwise one)
FAMILY_ENTRIES = ('t3d_dwconv_fwd', 't3d_dwconv_bwd', 't3d_expdw_fwd', 't3d_pwconv_fwd', 't3d_pwconv_fwd_mat', 't3d_pwconv_dgrad', 't3d_pwconv_wgrad',
                  't3d_pwconv_dgrad_yfree', 't3d_pwconv_wgrad_yfree', 't3d_pwconv_bwd_yfree', 't3d_pwconv_bwd_yfree_w')
MFMA_PEAK = 2.5e15         # FLOP/s, dense bf16 MFMA (same guide; fp32 storage runs v_mfma_f32_16x16x4_f32: 157 TFLOP/s)
MFMA_PEAK_F32 = 157.3e12
# PMC family (tools/pmc_traffic.sh groups by rocprof kernel name) -> the entry points whose launches it holds
PMC_GROUPS = {'t3d_dwconv_fwd': ('t3d_dwconv_fwd',), 't3d_dwconv_bwd': ('t3d_dwconv_bwd',),
              't3d_pwconv_fwd': ('t3d_pwconv_fwd', 't3d_pwconv_fwd_mat'), 't3d_pwconv_dgrad': ('t3d_pwconv_dgrad',),
              't3d_pwconv_wgrad': ('t3d_pwconv_wgrad',), 't3d_pwconv_dgrad_yfree': ('t3d_pwconv_dgrad_yfree',),
              't3d_pwconv_wgrad_yfree': ('t3d_pwconv_wgrad_yfree', 't3d_pwconv_bwd_yfree', 't3d_pwconv_bwd_yfree_w')}
# (entry point, k, stride) -> kernel name as rocprofv3 prints it (csrc/dwconv3_stream.hip, dwconv3_bwd_stream.hip,
# dwconvk_stream.hip, dwconv5_bwd_stream.hip, dwconv_bwd.hip), bf16 storage
DW_KERNEL_NAMES = {('t3d_dwconv_fwd', 3, 1): 'dw3_fwd2_kernel', ('t3d_dwconv_fwd', 3, 2): 'dw3_fwd_kernel',
                   ('t3d_dwconv_bwd', 3, 1): 'dw3_bwd2_kernel', ('t3d_dwconv_bwd', 3, 2): 'dw3_bwd_s2_kernel',
                   ('t3d_dwconv_fwd', 5, 1): 'dwk_fwd_kernel<5,1>', ('t3d_dwconv_fwd', 5, 2): 'dwk_fwd_kernel<5,2>',
                   ('t3d_dwconv_bwd', 5, 1): 'dw5_bwd_s1_kernel', ('t3d_dwconv_bwd', 5, 2): 'dw5_bwd_s2_kernel'}


def spawn_ranks(args):
    """`python bench.py --gpus N` run plainly (no launcher environment): start the N ranks ourselves as a CHILD
    process (`python -m torch.distributed.run`, one rank per GPU over RCCL) before anything in this process touches
    the GPU, pass its output through and exit with its code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={args.gpus}',
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    sys.exit(subprocess.run(cmd, env=env).returncode)


def device_warmup(dev, seconds=None):
    """Keeps the GPU busy with device-to-device copies for ~`seconds` (clock / power-state ramp of a fresh box); returns
    the seconds spent.  T3D_DEVICE_WARMUP_S overrides (0 disables)."""
    seconds = float(os.environ.get('T3D_DEVICE_WARMUP_S', 2.0)) if seconds is None else seconds
    if seconds <= 0:
        return 0.0
    a = torch.empty(64 << 20, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(20):
            b.copy_(a)
            a.copy_(b)
        torch.cuda.synchronize(dev)
    return round(time.perf_counter() - t0, 2)


def api_objects(args, dev):
    """The step as scripts/main.py of the reference builds it (main.py:46-82): build_model -> build_optimizer ->
    build_loss / LossManager -> Trainer; `Trainer.train_step` is the loop body of trainer/train.py:42-66.  Under a
    multi-rank launch `build_model(...).to(dev)` attaches the RCCL gradient exchange by itself."""
    from torchdet3d.builders import build_loss, build_model, build_optimizer
    from torchdet3d.losses import LossManager
    from torchdet3d.trainer import Trainer
    from torchdet3d.utils.utils import AttrDict
    cfg = AttrDict(dict(
        model=dict(name=args.model, num_classes=9, pretrained=False, load_weights='', storage_dtype=args.dtype,
                   eval_storage_dtype=args.eval_dtype or None),
        data=dict(normalization=dict(mean=[0.5931, 0.4690, 0.4229], std=[0.2471, 0.2214, 0.2157])),
        data_parallel=dict(use_parallel=False),
        optim=dict(name='adam', lr=1e-3, wd=1e-4, betas=(0.9, 0.999)),          # default_config.py:18
        loss=dict(names=['l1', 'add_loss', 'cross_entropy'], coeffs=([1., .1], [.2]), smoothl1_beta=0.2, w=5.18, eps=1.,
                  alwa=dict(use=False, lam_cls=1., lam_reg=1., C=100, compute_std=True))))      # default_config.py:22
    model = build_model(cfg).to(dev)
    model.net.reset_parameters(seed=5)
    if model.grad_sync is not None:              # the seeded weights of rank 0 everywhere
        model.grad_sync.broadcast([model.net.flat] + list(model.net.buffers.values()))
    opt = build_optimizer(cfg, model)
    lm = LossManager(build_loss(cfg), cfg.loss.coeffs, cfg.loss.alwa)
    tr = Trainer(model, None, opt, None, lm, None, 1, '', device=dev, save_chkpt=False)
    model.train()
    if args.eval:
        # the validation loop's body (evaluation/evaluate.py:88-95): eval-mode forward + per-class metrics incl. the 3-D IoU
        from torchdet3d.evaluation import Evaluator
        model.eval()
        return model, Evaluator(model=model, val_loader=None, cfg=cfg, device=dev)
    return model, tr


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--model', default='mobilenetv2')
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'f32'])
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--cpu-batch', type=int, default=32)
    ap.add_argument('--cpu-threads', type=int, default=0, help='host threads of the CPU leg (0: the count the recorded sweep '
                    'found fastest, profiles/r5_cpu_baseline_thread_sweep.txt, capped by the host)')
    ap.add_argument('--cpu-steps', type=int, default=60)
    ap.add_argument('--cpu-baseline-only', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--eval', action='store_true', help='time the validation step instead of the train step: `Evaluator.val_step` '
                    'of a model built by build_model (eval-mode forward on the engine `model.eval_storage_dtype` selects -- fp32 '
                    'storage by default, also for a bf16 model -- + ADD / SADD / accuracy / 3-D IoU per class)')
    ap.add_argument('--eval-sync', action='store_true', help='--eval: time Evaluator.val_step (waits for its own batch) instead of the '
                    "validation loop's pipelined body (Evaluator.val: one batch in flight)")
    ap.add_argument('--eval-dtype', default='', choices=['', 'bf16', 'f16', 'f32'], help="model.eval_storage_dtype for --eval; 'bf16' is "
                    'the OPT-IN throughput inference, outside the 1e-3 3-D-IoU bound for MobileNetV2 (labelled in the output)')
    ap.add_argument('--engine', action='store_true', help='drive models.engine.Net + the loss / optimizer kernels directly '
                    'instead of going through the reference-shaped API (build_model / build_optimizer / LossManager / '
                    'Trainer.train_step), which is what the headline number is measured through')
    ap.add_argument('--roofline-every', type=int, default=4, help='--full: the depthwise launches of every n-th timed step carry '
                    'HIP-event pairs (an event pair per launch on all steps costs ~0.25 ms per step)')
    ap.add_argument('--per-launch', action='store_true', help='print every conv launch of one step (stderr)')
    ap.add_argument('--profile-all', action='store_true', help='time every kernel family, print a table to stderr')
    ap.add_argument('--full', action='store_true', help='also measure what the headline figure does not need: the host issue '
                    'time of a step (two extra untimed steps), the roofline block (HIP-event pairs on the convolution launches '
                    'of sampled timed steps) and the CPU baseline (a child process of up to 150 s; --no-cpu-baseline drops it)')
    ap.add_argument('--dump-outputs', metavar='DIR', default='', help='after the timed steps, write what the last of them '
                    'computed as DIR/<name>.npy (float32 / float64; an array of more than %d elements as a fixed, seeded '
                    'sample of them)' % DUMP_MAX_ELEMS)
    return ap.parse_args()


CPU_THREADS_BEST = 16     # profiles/r5_cpu_baseline_thread_sweep.txt: B = 32 train step of the oracle at 8 / 16 / 32 / 64 / 128 threads: 50.6 / 53.0 / 40.4 / 18.8 / 8.7 crops/s


def cpu_baseline(model, size, batch, steps, budget_s=25.0, threads=0):
    """The oracle's train step (fwd + losses + autograd bwd + AdamW) on the host cores, on a BOUNDED sample:
    at most `steps` steps and ~`budget_s` seconds, batch 32.  Thread count: the fastest of a one-off
    sweep on the GPU box's host (recorded under profiles/): with every hardware thread of a 256-thread host the small
    convolutions of this network oversubscribe and run ~50x slower."""
    from oracle import losses as OL
    from oracle import model as OMod
    from oracle.weights import make_inputs, make_state_dict
    cores = min(os.cpu_count() or 1, threads or CPU_THREADS_BEST)
    torch.set_num_threads(cores)
    sd = make_state_dict(model, 9)
    params = {k: v.clone().requires_grad_(v.dtype.is_floating_point and 'running' not in k) for k, v in sd.items()}
    opt = torch.optim.AdamW([p for p in params.values() if p.requires_grad], lr=1e-3, weight_decay=1e-4)
    lm = OL.LossManager(OL.build(['l1', 'add_loss', 'cross_entropy']), ([1., .1], [.2]))
    imgs, gt, cats = make_inputs(batch, size, size, 9)
    mask = (torch.rand(batch, 1280) >= 0.5).float() * 2

    def step():
        kp, tg = OMod.forward(params, model, imgs, cats, train=True, num_classes=9, dropout_mask=mask)
        loss = lm.parse_losses(kp, gt, tg, cats, 0)
        opt.zero_grad()
        loss.backward()
        opt.step()

    t0 = time.perf_counter()
    step()                                   # warm-up (also the only sample if the host is very slow)
    warm = time.perf_counter() - t0
    done, dt = 0, 0.0
    t0 = time.perf_counter()
    while done < steps and warm + dt + (dt / done if done else warm) < budget_s:
        step()
        done += 1
        dt = time.perf_counter() - t0
    if done == 0:
        done, dt, note = 1, warm, 'the warm-up step itself (host too slow for more inside the time budget)'
    else:
        note = f'{done} train steps after 1 warm-up step'
    return dict(value=round(batch * done / dt, 2), unit='crops/s', cores=cores, kind='port',
                sample=f'{note}: {model} at batch {batch}, {size}x{size}, fp32 '
                       f'({warm + dt:.1f} s of CPU work, torch {torch.__version__} CPU kernels, {cores} threads of '
                       f'{os.cpu_count()})')


def cpu_baseline_guarded(args):
    """Runs the CPU leg in a child process with a hard wall-clock limit, so that a slow or oversubscribed host can
    never stall the benchmark (the child never touches the GPU)."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), '--cpu-baseline-only', '--model', args.model, '--size', str(args.size),
           '--cpu-batch', str(args.cpu_batch), '--cpu-steps', str(args.cpu_steps), '--cpu-threads', str(args.cpu_threads)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=150)
        return json.loads(out.stdout.strip().split('\n')[-1])
    except Exception as e:  # noqa: BLE001  (timeout, crash, unparsable output)
        return dict(value=None, unit='crops/s', cores=min(os.cpu_count() or 1, args.cpu_threads or CPU_THREADS_BEST), kind='port',
                    sample=f'CPU leg did not finish within its 150 s limit ({type(e).__name__})')


DUMP_MAX_ELEMS = 1 << 22    # per array (16 MB in float32): the largest model's weights and gradient stay under 64 MB in all


def dump_outputs(d, arrays):
    """--dump-outputs: each array as d/<name>.npy, float64 where the value is (host floats, integer counters), float32 otherwise.
    An array of more than DUMP_MAX_ELEMS elements is written as the same seeded sample of its flattened elements on every run."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    for name, a in arrays.items():
        if torch.is_tensor(a):
            a = a.detach().cpu()
            a = (a.float() if a.is_floating_point() and a.dtype != torch.float64 else a.double()).numpy()
        else:
            a = np.asarray(a, dtype=np.float64)
        if a.size > DUMP_MAX_ELEMS:
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, DUMP_MAX_ELEMS, replace=False))]
        np.save(os.path.join(d, name + '.npy'), a)


def conv_source_hash():
    """sha256 (16 hex digits) over every source of the HIP library: a committed PMC pass is quoted only for the kernels it saw."""
    import hashlib
    h = hashlib.sha256()
    cs = os.path.join(ROOT, '3d-object-detection.pytorch_amd', 'csrc')
    for f in sorted(x for x in os.listdir(cs) if x.endswith(('.hip', '.h'))):
        h.update(open(os.path.join(cs, f), 'rb').read())
    return h.hexdigest()[:16]


def pmc_families(args, S, B):
    """HBM bytes per step and PMC family from the latest committed rocprofv3 counter pass (tools/pmc_traffic.sh), or {} when it
    was collected on another workload or on other kernel sources."""
    import glob
    tfs = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r[0-9]*_hbm_traffic_pmc.json')))
    if not tfs or not (args.model == 'mobilenetv2' and S == 224 and B == 256 and args.dtype == 'bf16' and not args.eval):
        return {}
    pm = json.load(open(tfs[-1]))
    if pm.get('conv_source_sha256') != conv_source_hash():
        return {'_source': 'stale'}
    out = {k: v['hbm_bytes_per_step'] for k, v in pm.get('families', {}).items()}
    out['_source'] = f"profiles/{os.path.basename(tfs[-1])} (committed rocprofv3 --pmc pass at {pm.get('commit', '?')})"
    return out


def family_block(launches, nsteps, args, pmc):
    """roofline.families: every convolution entry point of the step, each launch timed on its own dispatch (begin-to-end of the
    kernel, as rocprofv3 reports it) inside the timed region, on `nsteps` of its steps.  Per family: launches and device time
    per step, algorithmic HBM bytes (input + output once per pass) and GEMM FLOPs, both as a fraction of
    the chip's peak; `counter_ratio` = HBM bytes of the rocprofv3 PMC pass / algorithmic bytes, for the PMC family the entry
    point belongs to.  `worst` = the family (>= 2 % of the summed conv time) with the lowest fraction of the roof that bounds it."""
    peak_f = MFMA_PEAK if args.dtype == 'bf16' else MFMA_PEAK_F32
    groups = {}
    for name, sig, ms, nby in launches:
        if not (ms > 5e-4):                 # (an entry point whose path had no timed launch site: recorded back to back)
            continue
        d = groups.setdefault(name, dict(launches=0, ms=0.0, bytes=0, flops=0.0))
        d['launches'] += 1
        d['ms'] += ms
        d['bytes'] += nby or 0
        if name.startswith('t3d_pwconv') and len(sig) >= 4:
            m_, k_, n_ = sig[-4], sig[-2], sig[-1]
            d['flops'] += 2.0 * m_ * k_ * n_ * (2 if 'bwd_yfree' in name else 1)    # (the fused pass: data gradient + weight-gradient products)
        elif name.startswith('t3d_dwconv') and len(sig) >= 6:
            b_, h_, w_, c_, kk, st_ = sig[-6:]
            d['flops'] += 2.0 * b_ * ((h_ - 1) // st_ + 1) * ((w_ - 1) // st_ + 1) * c_ * kk * kk * (2 if name.endswith('bwd') else 1)
    total_ms = sum(d['ms'] for d in groups.values()) or 1.0
    rows = []
    for name, d in groups.items():
        t = d['ms'] * 1e-3
        hb, mf = d['bytes'] / t / HBM_PEAK, d['flops'] / t / peak_f
        rows.append({'entry': name, 'launches_per_step': d['launches'] // nsteps, 'ms_per_step': round(d['ms'] / nsteps, 4),
                     'algorithmic_MB_per_step': round(d['bytes'] / nsteps / 1e6, 1), 'achieved_GBps': round(d['bytes'] / t / 1e9, 1),
                     'hbm_frac': round(hb, 4), 'GFLOP_per_step': round(d['flops'] / nsteps / 1e9, 1), 'mfma_frac': round(mf, 4),
                     'bound': 'hbm' if hb >= mf else 'mfma', 'frac': round(max(hb, mf), 4), 'counter_ratio': None,
                     'share_of_conv_time': round(d['ms'] / total_ms, 4)})
    for fam, members in PMC_GROUPS.items():
        alg = sum(r['algorithmic_MB_per_step'] for r in rows if r['entry'] in members) * 1e6
        if fam in pmc and alg > 0:
            for r in rows:
                if r['entry'] in members:
                    r['counter_ratio'] = round(pmc[fam] / alg, 3)
    rows.sort(key=lambda r: r['frac'])
    cand = [r for r in rows if r['share_of_conv_time'] >= 0.02] or rows
    w = cand[0]
    return {'families': rows, 'families_sampled_steps': nsteps, 'families_counter_source': pmc.get('_source'),
            'families_note': 'in-step, kernel-exact HIP events on each launch\'s own dispatch; second-stream launches (weight gradients) '
                             'include the time their workgroups wait for the main stream\'s persistent kernels to free registers',
            'worst': {'entry': w['entry'], 'bound': w['bound'], 'frac': w['frac'], 'ms_per_step': w['ms_per_step'],
                      'counter_ratio': w['counter_ratio']}}


def main():
    args = parse()
    if args.cpu_baseline_only:
        print(json.dumps(cpu_baseline(args.model, args.size, args.cpu_batch, args.cpu_steps, threads=args.cpu_threads)), flush=True)
        return
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        spawn_ranks(args)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if world != args.gpus:
        raise SystemExit(f'bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks')
    if torch.cuda.device_count() < world:
        raise SystemExit(f'bench.py: --gpus {args.gpus} but only {torch.cuda.device_count()} GPU(s) visible')
    import torch.distributed as dist
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    if world > 1 or 'RANK' in os.environ:      # launched by torch.distributed.run (also with one rank)
        dist.init_process_group('nccl', device_id=dev)

    from torchdet3d import _native as N
    from torchdet3d.builders.optim_builder import FusedAdamW
    from torchdet3d.models.engine import Net
    from torchdet3d.parallel import GradSync

    B, S = args.batch, args.size
    dtype = torch.bfloat16 if args.dtype == 'bf16' else torch.float32
    use_api = not args.engine
    torch.manual_seed(5)
    if use_api:
        model, trainer = api_objects(args, dev)
        net = model.net
    else:
        net = Net(args.model, 9, dev, dtype)
        net.reset_parameters(seed=5)
        sync = GradSync(net.gflat)
        sync.broadcast([net.flat] + [b for b in net.buffers.values()])
        if world > 1 or sync.force:
            net.grad_hook = sync.ready
        flat = torch.nn.Parameter(net.flat)          # one hand-written AdamW launch over the flat master weights
        flat.grad = net.gflat
        # default_config.py:18 (lr 1e-3, wd 1e-4); the 1/world of the gradient average rides on the optimizer's gradient load
        opt = FusedAdamW([flat], lr=1e-3, weight_decay=1e-4, grad_scale=1.0 / world)

    g = torch.Generator(device=dev).manual_seed(5 + rank)
    nb = 2                                       # synthetic batches resident in HBM, cycled
    imgs = [torch.randn(B, 3, S, S, device=dev, generator=g) for _ in range(nb)]
    gts = [torch.rand(B, 18, device=dev, generator=g) for _ in range(nb)]
    cats = [torch.randint(0, 9, (B,), device=dev, generator=g) for _ in range(nb)]
    cfg = N.LossCfg()
    cfg.c_l1, cfg.c_add, cfg.c_ce = 1.0, 0.1, 0.2
    cfg.smoothl1_beta, cfg.wing_w, cfg.wing_eps, cfg.lam_reg, cfg.lam_cls = 0.2, 5.18, 1.0, 1.0, 1.0
    out = torch.zeros(16, device=dev)
    dkp, dlg = torch.empty(B, 18, device=dev), torch.empty(B, 9, device=dev)

    last = [None]
    pend = [None]              # --eval: the validation batch in flight

    def eval_step(i):
        j = i % nb
        if use_api:
            # (trainer = the Evaluator)  the body of `Evaluator.val`'s loop: batch i's metrics are read back after batch i + 1
            # is enqueued; --eval-sync: `Evaluator.val_step`, which waits for its own batch
            if args.eval_sync:
                last[0] = trainer.val_step(imgs[j], gts[j].view(B, 9, 2), cats[j], compute_iou=True)
                return
            cur = trainer.val_enqueue(imgs[j], gts[j].view(B, 9, 2), cats[j], compute_iou=True)
            if pend[0] is not None:
                last[0] = pend[0].result()
            pend[0] = cur
            return
        kp, lg = net.forward(imgs[j], cats[j], train=False)
        N.call('t3d_loss_fwd_bwd', cfg, N.ptr(kp), N.ptr(gts[j]), N.ptr(lg), N.ptr(cats[j]), N.ptr(out), None, None, B, 9,
               N.stream())
        last[0] = (kp, lg)

    def step(i):
        if args.eval:
            return eval_step(i)
        j = i % nb
        if use_api:
            last[0] = trainer.train_step(imgs[j], gts[j].view(B, 9, 2), cats[j], i)
            return
        kp, lg = net.forward(imgs[j], cats[j], train=True)
        N.call('t3d_loss_fwd_bwd', cfg, N.ptr(kp), N.ptr(gts[j]), N.ptr(lg), N.ptr(cats[j]), N.ptr(out), N.ptr(dkp),
               N.ptr(dlg), B, 9, N.stream())
        sync.start()
        net.backward(dkp, dlg)
        sync.finish(scale=False)
        opt.step()
        last[0] = (kp, lg)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- warm-up (untimed).  With --profile-all the second half of it times every kernel family, the weight gradients
    # on the main stream for those steps (event pairs on the second stream would also count the time a launch waits
    # for the main stream's persistent kernels to free registers, not just the kernel)
    fam = {}
    side = net._side
    # device warm-up ahead of the W warm-up steps: the first process on a fresh box sometimes ran its whole timed region
    # 12-15 % slow (9.5-10.2 instead of 8.4-8.5 ms/step; never a later process) -- clock / power state still ramping.  About two
    # seconds of plain HBM copy kernels first (NOT steps of the workload: `warmup` below is the true number of untimed steps);
    # the W warm-up steps and the K timed steps follow.
    device_warmup_s = device_warmup(dev)
    for i in range(args.warmup):
        if args.profile_all and i == max(1, args.warmup // 2):
            N.timer = N.KernelTimer(None)
            net._side = None
        step(i)
    if N.timer is not None:
        fam = N.timer.summary()
        N.timer = None
    net._side = side
    # host cost of a step: time to ENQUEUE two steps into an empty queue (inside the timed region the host runs ahead
    # until HIP's queue back-pressure stalls it, which would be measured instead)
    t_issue = None
    if args.full:
        barrier()
        t0 = time.perf_counter()
        step(0)
        step(1)
        t_issue = (time.perf_counter() - t0) / 2
    if args.profile_all and rank == 0:
        tot = sum(v['ms'] for v in fam.values())
        for k, v in sorted(fam.items(), key=lambda kv: -kv[1]['ms']):
            bw = v['bytes'] / (v['ms'] * 1e-3) / 1e12 if v['ms'] > 0 and v['bytes'] else 0
            print(f'  {k:22s} {v["launches"]:5d} launches {v["ms"]:9.3f} ms {100 * v["ms"] / tot:5.1f}%  '
                  f'{bw:6.2f} TB/s algorithmic', file=sys.stderr)

    if args.per_launch and rank == 0:
        N.timer = N.KernelTimer(set(CONV_KERNELS))
        step(0)
        for n, sg, ms, nby in N.timer.per_launch():
            print(f'  {n:20s} {str(sg):44s} {ms * 1e3:8.1f} us  {(nby or 0) / 1e6:8.1f} MB  {(nby or 0) / ms / 1e9:6.2f} TB/s',
                  file=sys.stderr)
        N.timer = None

    # ---- timed region: exactly K steps; with --full the depthwise launches (main stream) carry HIP-event pairs
    every = max(1, args.roofline_every)
    # ... and on three steps spread over the region EVERY convolution launch does (roofline.families): ~200 pairs per step cost
    # ~1 ms on that step, so it is three steps and not every 4th
    full_steps = sorted({args.steps // 4, args.steps // 2, (3 * args.steps) // 4}) if args.steps >= 8 else [0]
    # kernel_exact: the event pair is attached to the depthwise kernel's own dispatch (begin-to-end of the kernel, as rocprofv3
    # reports it), not recorded around the launch call (which adds 5-9 us of event packets and dispatch latency)
    rtimer = (N.KernelTimer(set(DW_ENTRIES), prealloc=2 * 40 * ((args.steps + every - 1) // every), kernel_exact=not os.environ.get('T3D_EVENTS_AROUND'))
              if args.full else None)
    N.timer = None
    # the API path replays a recorded step plan (trainer/step_plan.py: one t3d_plan_run per step): the event pairs are then
    # attached by the replay itself, to the same launches through the same t3d_set_launch_events
    sp = trainer._step_plan() if (use_api and not args.eval) else None
    replayed = sp is not None and sp.rec is not None
    ptimer = None
    if args.full and replayed:
        from torchdet3d.trainer.step_plan import PlanTiming
        ncalls = lambda names: sum(1 for c in sp.rec.calls if c[0] in names)
        ptimer = sp.timing = PlanTiming(sp, {'dw': DW_ENTRIES, 'all': FAMILY_ENTRIES},
                                        ncalls(DW_ENTRIES) * ((args.steps + every - 1) // every) + ncalls(FAMILY_ENTRIES) * len(full_steps))
    # no cyclic-GC pass inside the timed region: one in three fresh processes had a single 36-44 ms step in it
    # (config.step_ms_min_med_max), i.e. +12 % on the 30-step average, from a collection over the freshly imported heap
    import gc
    gc.collect()
    gc.disable()
    barrier()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]   # step boundaries on the main stream
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(args.steps):
        if ptimer is not None:
            ptimer.select('all' if i in full_steps else ('dw' if i % every == 0 else None))
        else:
            N.timer = rtimer if i % every == 0 else None
        step(i)
        marks[i + 1].record()
    if pend[0] is not None:                      # --eval: the last batch's read-back belongs to the timed region
        last[0], pend[0] = pend[0].result(), None
    N.timer = None
    barrier()
    dt = time.perf_counter() - t0
    gc.enable()
    fam_launches, fam_steps, launches, nsampled = [], 0, [], 0
    if ptimer is not None:
        ptimer.close()
        sp.timing = None
        fam_launches, fam_steps = ptimer.per_launch('all'), ptimer.steps('all')
        launches, nsampled = ptimer.per_launch('dw'), ptimer.steps('dw')
    elif rtimer is not None:
        launches, nsampled = rtimer.per_launch(), (args.steps + every - 1) // every
    per_step = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    loss = (last[0][1] if args.eval else last[0]['loss']) if use_api else out[0].item()      # (--eval through the API: the batch's ADD)
    assert loss == loss or os.environ.get('T3D_ABLATE'), 'loss is NaN'
    # (the clamp-form ReLU6 of the 16-bit kernels maps a NaN pre-activation to 0: a diverged step is seen in the BatchNorm sums)
    assert args.eval or not net.nonfinite() or os.environ.get('T3D_ABLATE'), 'a BatchNorm saw non-finite batch sums'
    if args.dump_outputs and rank == 0:
        # what the caller of the timed path holds after its last step: the returned metrics (the API path) or the engine's
        # outputs, and after a train step the updated master weights, their gradient and the BatchNorm running statistics
        if args.eval and use_api:
            arrays = {'per_class_metrics': [list(r) for r in last[0][0]], 'metrics': last[0][1:]}
        elif use_api:
            arrays = {'metrics': [last[0][k] for k in ('loss', 'ADD', 'SADD', 'acc')]}
        else:
            arrays = {'keypoints': last[0][0], 'logits': last[0][1], 'loss_terms': out}
        if not args.eval:
            arrays.update(weights=net.flat, grads=net.gflat,
                          bn_buffers=torch.cat([b.double().reshape(-1) for b in net.buffers.values()]))
        dump_outputs(args.dump_outputs, arrays)

    eval_dt = None
    if args.eval:
        eval_dt = {torch.bfloat16: 'bf16', torch.float16: 'f16', torch.float32: 'f32'}[model.net_eval.dtype] if use_api else args.dtype
    if rank == 0:
        crops = B * world * args.steps / dt
        res = {
            'metric': f'regression {"eval" if args.eval else "train"} crops/sec @{S}^2 bs{B} ' + {'mobilenetv2': 'MobileNetV2', 'mobilenetv3_large': 'MobileNetV3-large', 'mobilenetv3_small': 'MobileNetV3-small', 'resnet50': 'ResNet-50'}.get(args.model, args.model), 'value': round(crops, 1), 'unit': 'crops/s',
            'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': round(dt / args.steps * 1e3, 3),
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': eval_dt if args.eval else args.dtype, 'data': 'synthetic',
            'config': {'workload': f'{args.model} 9-class Objectron keypoint regression, '
                                   + ((f'validation step ({"Evaluator.val_step" if args.eval_sync else "the body of Evaluator.val, one batch in flight"}: '
                                       f'eval-mode forward in {eval_dt} storage + per-class ADD / SADD / '
                                       'accuracy / 3-D IoU, one read-back per batch)' if use_api else
                                       'inference forward (running BatchNorm statistics) + loss / metric values')
                                      if args.eval else
                                      f'train step (fwd + l1/add/CE losses + bwd + AdamW{" + RCCL grad all-reduce" if world > 1 else ""})')
                                   + f', {S}x{S} crops, per-GPU batch {B}', 'global_batch': B * world, 'parallelism': f'dp{world}',
                       'final_loss': round(loss, 5), 'host_issue_ms_per_step': round(t_issue * 1e3, 3) if t_issue is not None else None,
                       'driven_through': ((('torchdet3d.builders.build_model / Evaluator.val_step' if args.eval_sync else 'torchdet3d.builders.build_model / Evaluator.val_enqueue + PendingMetrics.result (= Evaluator.val)') if args.eval else
                                           'torchdet3d.builders.build_model / build_optimizer / LossManager / Trainer.train_step')
                                          if use_api else 'models.engine.Net + loss / optimizer entry points'),
                       'step_form': (('one t3d_plan_run call per step (recorded step plan: %d launches, %d stream forks)'
                                      % (N.lib().t3d_plan_num_ops(sp.rec.plan, 0), N.lib().t3d_plan_num_ops(sp.rec.plan, 1)))
                                     if replayed else
                                     ('eval-mode forward replayed from a recorded plan (one t3d_plan_run, %d launches) + the metric launches'
                                      % N.lib().t3d_plan_num_ops(model._forward_plan().rec.plan, 0))
                                     if (args.eval and use_api and getattr(model._forward_plan(), 'rec', None) is not None) else
                                     'one host call per launch'),
                       'roofline_sampled_steps': nsampled,
                       'device_warmup_s': device_warmup_s, 'step_ms_min_med_max': [round(per_step[0], 3), round(per_step[len(per_step) // 2], 3), round(per_step[-1], 3)], 'side_stream_probe': list(__import__('torchdet3d.models.engine', fromlist=['x'])._concurrent_stream.log), 'rccl_ranks': world if dist.is_initialized() else 0},
        }
        # per depthwise family: (entry, k, stride) from the launch's integer arguments (..., B, H, W, C, k, stride)
        groups = {}
        for name, sig, ms, nby in launches:
            key = (name, sig[-2], sig[-1])
            d = groups.setdefault(key, dict(launches=0, ms=0.0, bytes=0))
            d['launches'] += 1
            d['ms'] += ms
            d['bytes'] += nby or 0
        rows = []
        for key, d in sorted(groups.items(), key=lambda kv: -kv[1]['ms']):
            ach = d['bytes'] / (d['ms'] * 1e-3) / 1e9
            rows.append({'kernel': DW_KERNEL_NAMES.get(key, '?') if args.dtype == 'bf16' else f'{key[0]} k{key[1]} s{key[2]} (fp32)',
                         'entry': key[0], 'k': key[1], 'stride': key[2],
                         'launches_per_step': d['launches'] // nsampled,
                         'avg_launch_us': round(1e3 * d['ms'] / d['launches'], 2),
                         'ms_per_step': round(d['ms'] / nsampled, 4),
                         'algorithmic_MB_per_step': round(d['bytes'] / nsampled / 1e6, 1),
                         'achieved': round(ach, 1), 'frac': round(ach * 1e9 / HBM_PEAK, 4)})
        if rows:
            top = rows[0]
            # HBM bytes per launch of that family from the committed rocprofv3 PMC passes (FETCH_SIZE x2 + WRITE_SIZE,
            # gfx950 correction): not measurable from inside this process, so it is quoted with its source, and only
            # for the workload the passes were collected on
            traffic, tsrc = None, None
            import glob
            tfs = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r[0-9]*_hbm_traffic_pmc.json')))
            tf = tfs[-1] if tfs else ''                  # the latest round's committed PMC pass
            if tf and args.model == 'mobilenetv2' and S == 224 and B == 256 and args.dtype == 'bf16' and not args.eval:
                pm = json.load(open(tf))
                fam_t = pm.get('kernels', {}).get(top['kernel'])
                # the pass is only quoted while the depthwise kernels it was collected on are the ones in the tree: the file
                # carries the hash of csrc/dwconv3*_stream.hip at collection time (tools/pmc_traffic.sh); anything else is stale
                import hashlib
                h = hashlib.sha256()
                cs = os.path.join(ROOT, '3d-object-detection.pytorch_amd', 'csrc')
                for f in sorted(x for x in os.listdir(cs) if x.startswith('dwconv3') and x.endswith('_stream.hip')):
                    h.update(open(os.path.join(cs, f), 'rb').read())
                if fam_t and pm.get('dw3_source_sha256') == h.hexdigest()[:16]:
                    traffic = round(fam_t['hbm_bytes_per_step'] / top['launches_per_step'])
                    tsrc = f"profiles/{os.path.basename(tf)} (committed rocprofv3 --pmc pass at {pm.get('commit', '?')})"
                elif fam_t:
                    tsrc = 'stale'          # (traffic stays null: the depthwise sources changed since the last tools/pmc_traffic.sh pass)
            res['roofline'] = {'bound': 'hbm', 'kernel': top['kernel'], 'entry': top['entry'], 'achieved': top['achieved'],
                               'peak': HBM_PEAK / 1e9, 'unit': 'GB/s', 'frac': top['frac'], 'traffic': traffic,
                               'traffic_source': tsrc,
                               'traffic_note': ("per launch, all tensors the kernel touches (gradient, raw output and raw input read, input gradient "
                                                "written, halo columns / rows re-read) plus the flush of 11*C partial sums per workgroup") if traffic and top['kernel'] == 'dw3_bwd2_kernel' else None,
                               'launches_per_step': top['launches_per_step'],
                               'avg_launch_us': top['avg_launch_us'],
                               'algorithmic_MB_per_step': top['algorithmic_MB_per_step'],
                               'selection': 'depthwise family with the most device time over the timed steps',
                               'depthwise': rows}
        if fam_steps:
            res['roofline'] = res.get('roofline') or {'bound': 'hbm', 'peak': HBM_PEAK / 1e9, 'unit': 'GB/s'}
            res['roofline'].update(family_block(fam_launches, fam_steps, args, pmc_families(args, S, B)))
            if 'kernel' not in res['roofline']:
                # a model without depthwise layers (ResNet-50, BASELINE config 4: "stresses the MFMA dense-conv path"): the
                # headline entry is the GEMM family with the most device time, against the roof that bounds it
                top = max(res['roofline']['families'], key=lambda r: r['ms_per_step'])
                mf = top['bound'] == 'mfma'
                res['roofline'].update({'bound': top['bound'], 'entry': top['entry'], 'kernel': top['entry'],
                                        'achieved': round(top['mfma_frac'] * (MFMA_PEAK if args.dtype == 'bf16' else MFMA_PEAK_F32) / 1e12, 1) if mf else top['achieved_GBps'],
                                        'peak': ((MFMA_PEAK if args.dtype == 'bf16' else MFMA_PEAK_F32) / 1e12) if mf else HBM_PEAK / 1e9,
                                        'unit': 'TFLOP/s' if mf else 'GB/s', 'frac': top['frac'], 'traffic': None,
                                        'launches_per_step': top['launches_per_step'], 'ms_per_step': top['ms_per_step'],
                                        'selection': 'convolution family with the most device time over the sampled steps'})
        if args.model == 'mobilenetv2' and S == 224 and args.dtype == 'bf16':
            per_crop = 26.89 if args.eval else MNV2_TRAIN_MB_PER_CROP     # forward / train MB per crop
            if args.eval and eval_dt == 'f32':
                per_crop *= 2                                              # fp32 storage: 4 B per element
            res['config']['step_hbm_roofline_frac'] = round(crops / world * per_crop * 1e6 / HBM_PEAK, 4)
        if args.eval and eval_dt == 'bf16' and args.model == 'mobilenetv2':
            # the opt-in bf16 INFERENCE of this model is outside the north-star's 3-D-IoU bound: say so next to the number
            res['config']['parity_note'] = ('bf16 inference is NOT parity-gated: 3-D IoU deviates by 2e-3 (sigma 0.024) .. 4e-3 from the fp32 '
                                            'oracle (bound 1e-3; tests/test_gpu_bf16_gate.py); the default eval engine (fp32 storage) '
                                            'meets it')
        if args.full and world == 1 and not args.no_cpu_baseline and not args.eval:
            res['cpu_baseline'] = cpu_baseline_guarded(args)
        print(json.dumps(res), flush=True)
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
