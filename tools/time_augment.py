"""Cost of the Objectron input path (csrc/augment.hip, dataloaders/gpu_loader.py) on one GPU.

  1. HIP-event time of one `t3d_augment_crops_u8` launch at B = 164 and 256, 224x224 output, crop sizes drawn like Objectron
     boxes (150 - 500 px a side), all augmentations at the default config's rates; also with every sample rotated.
     With --chain also `t3d_augment_chain_crops_u8` (csrc/augment_chain.hip) on the same crops: the default pipeline plus
     hue_saturation_value, color_jitter and random_rescale, every transform at p = 1 (four launches a batch).
  2. Loader batches/s with num_workers 0 / 8 / 16 over a generated directory of 960x720 JPEGs (Pillow decode + crop in the
     workers, draws + upload + kernel in the main process), nothing else running.  256 JPEG files, `--objects` annotations
     cycling over them (every object decodes its frame, as Objectron does); the timing starts after the first batch.
  3. `Trainer.train(epoch)` crops/s (MobileNetV3-large, bf16, the default step plan) over the same loader.
Prints one JSON line per measurement.
Usage: python tools/time_augment.py [--objects N] [--batch B] [--workers 0,8,16] [--chain] [--kernels-only]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-object-detection.pytorch_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def kernel_time(B, rotate_all=False, reps=50, chain=False):
    from torchdet3d import _native as N
    from torchdet3d.dataloaders.objectron import AugmentPipeline, chain_scratch_bytes, chain_stages
    import augment_ref as R
    tr, _ = R.default_pipelines((224, 224))
    if chain:
        tr = tr[:4] + [('hue_saturation_value', dict()), ('color_jitter', dict()), ('random_rescale', dict(scale_limit=(0.8, 1.25))),
                       tr[4]] + tr[5:]
    if rotate_all or chain:
        tr = [(n, a if n in ('convert_color', 'resize', 'normalize', 'to_tensor') else dict(a, p=1.0)) for n, a in tr]
    pipe = AugmentPipeline(tr, R.NORMALIZATION)
    rng = np.random.default_rng(B)
    hw = rng.integers(150, 501, (B, 2))
    sizes = hw[:, 0] * hw[:, 1] * 3
    desc = np.stack([np.concatenate([[0], np.cumsum(sizes)[:-1]]), hw[:, 0], hw[:, 1]], 1).astype(np.int64)
    src = torch.randint(0, 256, (int(sizes.sum()),), dtype=torch.uint8, device='cuda')
    rec = pipe.records(desc, pipe.draw(B, (0, 0, 0, 0)))
    out = torch.empty(B, 224, 224, 3, dtype=torch.uint8, device='cuda')
    if chain:
        rec, ext = rec
        stages = chain_stages(rec, ext)
        extd = torch.from_numpy(ext.view(np.uint8).copy()).cuda()
        scratch = torch.empty(chain_scratch_bytes(B, 224, 224, stages), dtype=torch.uint8, device='cuda')
    recd = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    if chain:
        name = 't3d_augment_chain_crops_u8'
        args = (N.ptr(src), src.numel(), N.ptr(recd), N.ptr(extd), N.ptr(scratch), scratch.numel(), N.ptr(out), B, 224, 224, stages)
    else:
        name = 't3d_augment_crops_u8'
        args = (N.ptr(src), src.numel(), N.ptr(recd), N.ptr(out), B, 224, 224)
    for _ in range(5):
        N.call(name, *args, N.stream())
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        N.call(name, *args, N.stream())
        e1.record()
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
    return dict(what='kernel', entry=name, B=B, rotate_all=rotate_all or chain, median_us=round(t[len(t) // 2], 2),
                min_us=round(t[0], 2), max_us=round(t[-1], 2), crop_MB=round(src.numel() / 1e6, 1),
                out_MB=round(out.numel() / 1e6, 1))


def make_frames(root, n, files=256):
    from PIL import Image
    rng = np.random.default_rng(0)
    os.makedirs(os.path.join(root, 'annotations'), exist_ok=True)
    os.makedirs(os.path.join(root, 'img'), exist_ok=True)
    yy, xx = np.mgrid[0:720, 0:960]
    base = np.stack([127 + 100 * np.sin(xx / 23.0 + c) * np.cos(yy / 31.0 - c) for c in range(3)], -1)
    images, anns = [], []
    for i in range(files):
        frame = np.clip(base + rng.normal(0, 10, base.shape), 0, 255).astype(np.uint8)
        Image.fromarray(frame).save(os.path.join(root, 'img', f'{i}.jpg'), quality=90)
        images.append(dict(id=i, file_name=f'img/{i}.jpg', width=960, height=720))
    for i in range(n):
        c = rng.uniform([250, 250], [710, 470])
        half = rng.uniform(65, 240)
        kp = c + rng.uniform(-half, half, (9, 2))
        anns.append(dict(id=i, image_id=i % files, category_id=int(rng.integers(1, 10)), keypoints=[float(v) for v in kp.reshape(-1)]))
    import json as js
    for split in ('train', 'test'):
        with open(os.path.join(root, 'annotations', f'objectron_{split}.json'), 'w') as f:
            js.dump(dict(images=images, annotations=anns), f)


def cfg_for(root, B, workers):
    import augment_ref as R
    from test_host_logic import _cfg
    cfg = _cfg('mobilenetv3_large')
    tr, te = R.default_pipelines((224, 224))
    cfg.data = type(cfg)(dict(root=root, resize=(224, 224), train_batch_size=B, val_batch_size=B, num_workers=workers,
                              category_list='all', normalization=R.NORMALIZATION, max_epochs=1))
    cfg.utils = type(cfg)(dict(random_seeds=5))
    cfg.train_data_pipeline, cfg.test_data_pipeline = tr, te
    return cfg


def loader_rate(root, B, workers):
    from torchdet3d.builders import build_loader
    train = build_loader(cfg_for(root, B, workers))[0]
    train.sampler.set_epoch(0)
    it = iter(train)
    next(it)                           # worker start-up outside the timing
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    for _ in it:
        n += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dict(what='loader', workers=workers, B=B, batches=n, batches_per_s=round(n / dt, 2), crops_per_s=round(n * B / dt, 1))


def train_rate(root, B, workers):
    from torchdet3d.builders import build_loader, build_loss, build_model, build_optimizer
    from torchdet3d.losses import LossManager
    from torchdet3d.trainer import Trainer
    cfg = cfg_for(root, B, workers)
    model = build_model(cfg).to('cuda')
    opt = build_optimizer(cfg, model)
    lm = LossManager(build_loss(cfg), cfg.loss.coeffs, cfg.loss.alwa)
    train = build_loader(cfg)[0]
    tr = Trainer(model, train, opt, None, lm, None, 2, '', device='cuda', save_chkpt=False, print_freq=10 ** 6)
    tr.debug, tr.debug_steps = True, 4
    tr.train(0, False)                 # warm-up: plan recording
    tr.debug = False
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.train(1, True)                  # (includes the workers' start-up, as every epoch of main.py does)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n = len(train) * B
    return dict(what='train', workers=workers, B=B, crops=n, crops_per_s=round(n / dt, 1), replays=tr._sp.replays if tr._sp else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--objects', type=int, default=164 * 40)
    ap.add_argument('--batch', type=int, default=164)
    ap.add_argument('--workers', default='0,8,16')
    ap.add_argument('--train-workers', type=int, default=16)
    ap.add_argument('--chain', action='store_true', help='also time t3d_augment_chain_crops_u8, every transform at p = 1')
    ap.add_argument('--kernels-only', action='store_true', help='stop after the kernel timings (no frames, loader or training)')
    a = ap.parse_args()
    for B in (164, 256):
        for rot in (False, True):
            print(json.dumps(kernel_time(B, rot)), flush=True)
        if a.chain:
            print(json.dumps(kernel_time(B, chain=True)), flush=True)
    if a.kernels_only:
        return
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        make_frames(root, a.objects)
        print(json.dumps(dict(what='frames', objects=a.objects, seconds=round(time.perf_counter() - t0, 1))), flush=True)
        for w in [int(v) for v in a.workers.split(',')]:
            print(json.dumps(loader_rate(root, a.batch, w)), flush=True)
        print(json.dumps(train_rate(root, a.batch, a.train_workers)), flush=True)


if __name__ == '__main__':
    main()
