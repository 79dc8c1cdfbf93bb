"""Cost of the device crop cache (`cfg.data.cache = 'device'`: dataloaders/gpu_loader.py, t3d_augment_resized_u8) on one GPU,
beside the uncached loader and the resident-batch step, all in one run over the directory of 960x720 quality-90 JPEGs that
tools/time_augment.py generates (256 files, `--objects` annotations cycling over them).  For B = 164 and 256:

  kernel    HIP-event median of one `t3d_augment_resized_u8` launch beside `t3d_augment_crops_u8` on the same records (224x224,
            crops of 150 - 500 px a side, the default config's rates; also with every sample flipped, LUT-ed and rotated):
            5 warm-up launches, 50 timed.
  prefill   `fill_cache()` crops/s with num_workers 0 / 8 / 16 (decode + crop in the workers, one resize launch per batch).
  finish    main-thread milliseconds per batch in the cached `finish_cached` (draws, records, keypoints, one upload, one
            launch), and the share of `pipeline.draw` / `records` / `keypoints` in it.
  epoch     `Trainer.train(epoch)` crops/s (MobileNetV3-large, bf16, the default step plan) over a whole epoch from the
            cache, alternating with the uncached loader with `--train-workers` workers (which pays its workers' start-up in
            every epoch, as scripts/main.py does), `--reps` times each.
  resident  `Trainer.train_step` crops/s over batches of the same shape that are already on the device.
Prints one JSON line per measurement.  Usage: python tools/time_crop_cache.py [--objects N] [--workers 0,8,16] [--reps 3]"""
import argparse
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from time_augment import cfg_for, make_frames  # noqa: E402  (also puts the repository, the package and tests/ on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _events(fn, warm=5, reps=50):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
    return round(t[len(t) // 2], 2), round(t[0], 2)


def kernel_times(B, rotate_all=False):
    """Both kernels on the same records: the crops kernel on the crops, the resized kernel on the arena made from them."""
    from torchdet3d import _native as N
    from torchdet3d.dataloaders.objectron import AUG_SAMPLE_DTYPE, AugmentPipeline
    import augment_ref as R
    tr, _ = R.default_pipelines((224, 224))
    if rotate_all:
        tr = [(n, dict(a, p=1.0) if n in ('random_rotate', 'horizontal_flip', 'random_brightness_contrast') else a) for n, a in tr]
    pipe = AugmentPipeline(tr, R.NORMALIZATION)
    rng = np.random.default_rng(B)
    hw = rng.integers(150, 501, (B, 2))
    sizes = hw[:, 0] * hw[:, 1] * 3
    desc = np.stack([np.concatenate([[0], np.cumsum(sizes)[:-1]]), hw[:, 0], hw[:, 1]], 1).astype(np.int64)
    src = torch.randint(0, 256, (int(sizes.sum()),), dtype=torch.uint8, device='cuda')
    prm = pipe.draw(B, (0, 0, 0, 0))
    slot = 224 * 224 * 3
    where = np.stack([rng.permutation(B) * slot, np.full(B, 224), np.full(B, 224)], 1).astype(np.int64)
    plain = np.zeros(B, AUG_SAMPLE_DTYPE)
    plain['offset'], plain['h'], plain['w'] = desc[:, 0], desc[:, 1], desc[:, 2]
    up = lambda rec: torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    arena = torch.empty(B * slot, dtype=torch.uint8, device='cuda')
    N.call('t3d_augment_crops_u8', N.ptr(src), src.numel(), N.ptr(up(plain)), N.ptr(arena), B, 224, 224, N.stream())
    # arena slot k holds crop k; record j reads slot perm[j], so give the crops kernel the same crop
    order = where[:, 0] // slot
    rc, ra = up(pipe.records(desc[order], prm)), up(pipe.records(where, prm))
    oc = torch.empty(B, 224, 224, 3, dtype=torch.uint8, device='cuda')
    oa = torch.empty_like(oc)
    crops = lambda: N.call('t3d_augment_crops_u8', N.ptr(src), src.numel(), N.ptr(rc), N.ptr(oc), B, 224, 224, N.stream())
    resized = lambda: N.call('t3d_augment_resized_u8', N.ptr(arena), arena.numel(), N.ptr(ra), N.ptr(oa), B, 224, 224, N.stream())
    (cm, cmin), (rm, rmin) = _events(crops), _events(resized)
    return dict(what='kernel', B=B, rotate_all=rotate_all, crops_u8_median_us=cm, crops_u8_min_us=cmin, resized_u8_median_us=rm,
                resized_u8_min_us=rmin, equal=bool(torch.equal(oc, oa)), out_MB=round(oc.numel() / 1e6, 1))


def prefill_rate(root, B, workers):
    from torchdet3d.builders import build_loader
    cfg = cfg_for(root, B, workers)
    cfg.data.cache = 'device'
    train = build_loader(cfg)[0]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    train.fill_cache()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n = len(train.dataset)
    return train, dict(what='prefill', workers=workers, B=B, crops=n, seconds=round(dt, 2), crops_per_s=round(n / dt, 1),
                       arena_MB=round(train._arena.numel() / 1e6, 1))


def finish_cost(train, B):
    """Host time of the cached finish per batch (the main thread's share of an epoch), and of its three pipeline calls."""
    train.sampler.set_epoch(1)
    batches = [list(idx) for idx in train.loader.batch_sampler]
    for b, idx in enumerate(batches[:3]):
        train.finish_cached(idx, (b,))
    torch.cuda.synchronize()
    t_all, t_draw, t_rec, t_kp = [], [], [], []
    oh, ow = train.pipeline.size
    for b, idx in enumerate(batches):
        t0 = time.perf_counter()
        train.finish_cached(idx, (b,))
        t_all.append(time.perf_counter() - t0)
        ix = np.asarray(idx, np.int64)
        where = np.stack([ix * (oh * ow * 3), np.full_like(ix, oh), np.full_like(ix, ow)], 1)
        t0 = time.perf_counter()
        prm = train.pipeline.draw(len(ix), (train.seed, 1, train.rank, b))
        t1 = time.perf_counter()
        train.pipeline.records(where, prm)
        t2 = time.perf_counter()
        train.pipeline.keypoints(train._c_kp[ix], train._c_desc[ix], prm)
        t3 = time.perf_counter()
        t_draw.append(t1 - t0), t_rec.append(t2 - t1), t_kp.append(t3 - t2)
    torch.cuda.synchronize()
    ms = lambda v: round(_median(v) * 1e3, 3)
    return dict(what='finish_cached_host', B=B, batches=len(batches), median_ms=ms(t_all), mean_ms=round(np.mean(t_all) * 1e3, 3),
                draw_ms=ms(t_draw), records_ms=ms(t_rec), keypoints_ms=ms(t_kp))


def epochs(root, B, cached, workers, reps):
    from torchdet3d.builders import build_loader, build_loss, build_model, build_optimizer
    from torchdet3d.losses import LossManager
    from torchdet3d.trainer import Trainer
    cfg = cfg_for(root, B, workers)
    model = build_model(cfg).to('cuda')
    opt = build_optimizer(cfg, model)
    lm = LossManager(build_loss(cfg), cfg.loss.coeffs, cfg.loss.alwa)
    plain = build_loader(cfg)[0]
    tr = Trainer(model, cached, opt, None, lm, None, 2, '', device='cuda', save_chkpt=False, print_freq=10 ** 6)
    tr.debug, tr.debug_steps = True, 4
    tr.train(0, False)                 # warm-up: plan recording
    tr.debug = False
    out, n, epoch = [], len(cached) * B, 1
    for rep in range(reps):
        for name, loader in (('cached', cached), ('uncached', plain)):
            tr.train_loader = loader
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.train(epoch, False)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out.append(dict(what='train_epoch', loader=name, workers=0 if name == 'cached' else workers, B=B, rep=rep, crops=n,
                            seconds=round(dt, 3), crops_per_s=round(n / dt, 1)))
            epoch += 1
    # the step alone, on batches that are already on the device
    cached.sampler.set_epoch(0)
    res = []
    for b in cached:
        res.append(tuple(t.clone() for t in b))
        if len(res) == 8:
            break
    steps = len(cached)
    for i in range(5):
        tr.train_step(*res[i % len(res)], i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        tr.train_step(*res[i % len(res)], i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out.append(dict(what='train_step_resident', B=B, steps=steps, crops_per_s=round(steps * B / dt, 1),
                    ms_per_step=round(dt / steps * 1e3, 3), replays=tr._sp.replays if tr._sp else 0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--objects', type=int, default=164 * 40)
    ap.add_argument('--workers', default='0,8,16')
    ap.add_argument('--train-workers', type=int, default=16)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    say = lambda d: print(json.dumps(d), flush=True)
    for B in (164, 256):
        for rot in (False, True):
            say(kernel_times(B, rot))
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        make_frames(root, a.objects)
        say(dict(what='frames', objects=a.objects, seconds=round(time.perf_counter() - t0, 1)))
        for B in (164, 256):
            train = None
            for w in [int(v) for v in a.workers.split(',')] if B == 164 else [a.train_workers]:
                del train
                torch.cuda.empty_cache()
                train, r = prefill_rate(root, B, w)
                say(r)
            say(finish_cost(train, B))
            for r in epochs(root, B, train, a.train_workers, a.reps):
                say(r)


if __name__ == '__main__':
    main()
