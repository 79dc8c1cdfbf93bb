"""Cost of the device JPEG decode (csrc/jpeg.hip, dataloaders/jpeg.py) beside the host decode it replaces, on one GPU.

B generated frames of 1440 x 1920 (the generator of tools/time_detect_augment.py: a smooth random field plus noise, quality 90,
4:2:0), one JSON line per measurement:
  1. the index pass, files / s of one thread, and the index bytes per frame, for every seg_mcus of the sweep;
  2. device-event time of one `t3d_jpeg_decode_u8` call over the B frames (5 warm-up calls, then --reps timed: median, min,
     max) for seg_mcus in 2, 4, 8, 16, 32, 120 (120 = one MCU row of these frames);
  3. the upload of the B files' bytes beside the upload of the B raw frames, from pinned memory;
  4. Pillow's decode of one such file on one core;
  5. `GpuDetectionLoader` over a folder of these files (--epoch-frames items an epoch, batches of --loader-batch -- halved
     until the host-decoded batches the workers keep in flight fit into half of the free shared memory --, the config's train
     pipeline): batches / s of a whole epoch, worker start-up included, and batches / s from the first batch on, decode='host'
     (Pillow in the workers) alternating with decode='device', at 2 workers (the config) and at 16, --alternations times each;
     one line per epoch, then median and range per mode.
`--decode-only SEG` runs only 5 + --reps decode calls at one seg_mcus: the run to put under
`rocprofv3 --kernel-trace --stats` for the time of each launch.
Usage: python tools/time_jpeg_decode.py [--batch 80] [--reps 50] [--alternations 5] [--epoch-frames 960] [--loader-batch 16]
       [--parts decode,upload,pillow,loader] [--seg-mcus N] [--out FILE]"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-object-detection.pytorch_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, S = 1440, 1920, 300
SWEEP = (2, 4, 8, 16, 32, 120)
TRAIN_PIPELINE = [
    dict(type='LoadImageFromFile', to_float32=True),
    dict(type='LoadAnnotations', with_bbox=True),
    dict(type='PhotoMetricDistortion', brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18),
    dict(type='Expand', mean=[0, 0, 0], to_rgb=True, ratio_range=(1, 3)),
    dict(type='MinIoURandomCrop', min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.1),
    dict(type='Resize', img_scale=(S, S), keep_ratio=False),
    dict(type='Normalize', mean=[0, 0, 0], std=[255, 255, 255], to_rgb=True),
    dict(type='RandomFlip', flip_ratio=0.5),
    dict(type='DefaultFormatBundle'),
    dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels']),
]


def frame_jpeg(seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, (H // 16, W // 16, 3), dtype=np.uint8)
    img = np.asarray(Image.fromarray(small).resize((W, H), Image.BICUBIC)).astype(np.int16) + rng.integers(-8, 9, (H, W, 3))
    buf = io.BytesIO()
    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, format='JPEG', quality=90)
    return buf.getvalue()


def stats(ms, unit=1e3, suffix='us'):
    return {f'median_{suffix}': round(float(np.median(ms)) * unit, 1), f'min_{suffix}': round(min(ms) * unit, 1),
            f'max_{suffix}': round(max(ms) * unit, 1), 'reps': len(ms)}


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


class Decode:
    """The device side of one t3d_jpeg_decode_u8 call over `files`, tables uploaded once."""

    def __init__(self, files, seg_mcus):
        from torchdet3d.dataloaders import jpeg as J
        t0 = time.perf_counter()
        rows = [J.index_jpeg(f, seg_mcus) for f in files]
        self.index_s = time.perf_counter() - t0
        assert all(r[0] == 0 for r in rows)
        rows = [r[1:] for r in rows]
        sizes = np.array([len(f) for f in files], np.int64)
        frame = np.array([int(i['h']) * int(i['w']) * 3 for i, _ in rows], np.int64)
        self.plan = J.plan_batch(rows, np.cumsum(sizes) - sizes, sizes, np.cumsum(frame) - frame)
        self.index_bytes = (self.plan['infos'].nbytes + self.plan['segs'].nbytes) / len(files)
        self.data = torch.from_numpy(np.frombuffer(b''.join(files), np.uint8).copy()).cuda()
        self.tabs = [torch.from_numpy(self.plan[k].view(np.uint8).copy()).cuda() for k in ('infos', 'segs', 'items')]
        self.out = torch.empty(int(frame.sum()), dtype=torch.uint8, device='cuda')
        self.launch = J.launch_decode

    def __call__(self):
        self.status = self.launch(self.data, *self.tabs, self.plan, self.out)


def write_dataset(root, files, items):
    os.makedirs(os.path.join(root, 'annotations'), exist_ok=True)
    os.makedirs(os.path.join(root, 'images'), exist_ok=True)
    for i, f in enumerate(files):
        with open(os.path.join(root, f'images/{i:03d}.jpg'), 'wb') as fh:
            fh.write(f)
    rng = np.random.default_rng(1)
    images, anns = [], []
    for k in range(items):                      # an epoch walks the B files several times over
        images.append(dict(id=k + 1, file_name=f'images/{k % len(files):03d}.jpg', width=W, height=H))
        for _ in range(2):
            x, y = float(rng.uniform(0, W * .5)), float(rng.uniform(0, H * .5))
            anns.append(dict(id=len(anns), image_id=k + 1, category_id=int(rng.integers(1, 10)), iscrowd=0,
                             bbox=[x, y, float(rng.uniform(100, W * .45)), float(rng.uniform(100, H * .45))]))
    with open(os.path.join(root, 'annotations/objectron_train.json'), 'w') as f:
        json.dump(dict(images=images, annotations=anns, categories=[]), f)


def epoch_rate(root, decode, workers, B, seg_mcus):
    """One epoch -> (batches / s of the whole epoch, worker start-up and the first batch included; batches / s from the moment
    the first batch has arrived to the last; seconds until the first batch)."""
    from torchdet3d.dataloaders import DetectionAugmentPipeline, GpuDetectionLoader, ObjectronFrames
    ds = ObjectronFrames(root, 'train', decode=decode)
    if decode == 'device':
        ds.build_index(os.path.join(root, f'index{seg_mcus}.npy'), threads=16, seg_mcus=seg_mcus)
    loader = GpuDetectionLoader(ds, DetectionAugmentPipeline(TRAIN_PIPELINE, (S, S)), B, shuffle=True, num_workers=workers, drop_last=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n, t1 = 0, None
    for batch in loader:
        n += 1
        if t1 is None:
            torch.cuda.synchronize()
            t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return n / (t2 - t0), (n - 1) / (t2 - t1), t1 - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=80)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--alternations', type=int, default=5)
    ap.add_argument('--epoch-frames', type=int, default=960)
    ap.add_argument('--loader-batch', type=int, default=16)
    ap.add_argument('--decode-only', type=int, default=0)
    ap.add_argument('--parts', default='decode,upload,pillow,loader', help='which measurements to run')
    ap.add_argument('--seg-mcus', type=int, default=0, help='seg_mcus of the loader part (0: the default)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    from torchdet3d.dataloaders.jpeg import DEFAULT_SEG_MCUS
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(lines[-1] + '\n')
    B = a.batch
    files = [frame_jpeg(i) for i in range(B)]
    if a.decode_only:
        d = Decode(files, a.decode_only)
        timed(d, a.reps)
        assert not d.status.any().item()
        return
    parts = a.parts.split(',')
    emit(what='the generated frames', B=B, frame=[H, W], quality=90, sampling='4:2:0', jpeg_bytes_mean=int(np.mean([len(f) for f in files])))
    from PIL import Image
    if 'decode' in parts:
        want = np.asarray(Image.open(io.BytesIO(files[0])).convert('RGB'))
        best = None
        for seg in SWEEP:
            d = Decode(files, seg)
            ms = timed(d, a.reps)
            ok = not d.status.any().item() and bool((d.out[:want.size].cpu().numpy().reshape(want.shape) == want).all())
            emit(what='t3d_jpeg_decode_u8, one call over the batch', seg_mcus=seg, segments_per_frame=int(d.plan['max_segs']), equals_pillow=ok,
                 index_files_per_s_one_thread=round(B / d.index_s, 1), index_bytes_per_frame=int(d.index_bytes), **stats(ms))
            if best is None or np.median(ms) < best[1]:
                best = (seg, float(np.median(ms)))
            del d
        emit(what='best seg_mcus of the sweep', seg_mcus=best[0], median_us=round(best[1] * 1e3, 1), default=DEFAULT_SEG_MCUS)
    if 'upload' in parts:      # the files' bytes and the raw frames, from pinned memory
        hb = torch.from_numpy(np.frombuffer(b''.join(files), np.uint8).copy()).pin_memory()
        hf = torch.randint(0, 256, (B * H * W * 3,), dtype=torch.uint8).pin_memory()
        db, df = hb.cuda(), hf.cuda()
        for what, h_, d_ in (('upload of the file bytes from pinned memory', hb, db), ('upload of the raw frames from pinned memory', hf, df)):
            u = stats(timed(lambda: d_.copy_(h_, non_blocking=True), a.reps))
            emit(what=what, B=B, bytes=h_.numel(), GBps=round(h_.numel() / (u['median_us'] * 1e-6) / 1e9, 1), **u)
        del hb, hf, db, df
    if 'pillow' in parts:
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < 3.0:
            np.asarray(Image.open(io.BytesIO(files[n % B])).convert('RGB'))
            n += 1
        dt = time.perf_counter() - t0
        emit(what='Pillow decode of one 1440x1920 JPEG, one core', frames_per_s=round(n / dt, 1), ms_per_batch_of_B_on_one_core=round(B * dt / n * 1e3, 1))
    if 'loader' not in parts:
        return
    torch.cuda.empty_cache()
    seg = a.seg_mcus or DEFAULT_SEG_MCUS
    # the loader, host decode against device decode, alternating; one line per epoch, then the medians
    with tempfile.TemporaryDirectory() as root:
        write_dataset(root, files, a.epoch_frames)
        for workers in (2, 16):
            LB = a.loader_batch                   # the workers hand batches over through shared memory: 2 in flight per worker
            try:
                v = os.statvfs('/dev/shm')
                while LB > 1 and 2 * workers * LB * H * W * 3 > v.f_bavail * v.f_frsize // 2:
                    LB //= 2
            except OSError:
                pass
            rates = {'host': [], 'device': []}
            epoch_rate(root, 'device', workers, LB, seg)                # (builds and saves the index; not timed)
            for k in range(a.alternations):
                for mode in ('host', 'device'):
                    r = epoch_rate(root, mode, workers, LB, seg)
                    rates[mode].append(r)
                    emit(what='GpuDetectionLoader, one epoch', decode=mode, workers=workers, B=LB, batches=a.epoch_frames // LB, alternation=k,
                         batches_per_s_whole_epoch=round(r[0], 3), batches_per_s_after_the_first_batch=round(r[1], 3),
                         s_until_the_first_batch=round(r[2], 3))
            for j, what in ((0, 'whole epoch, start-up included'), (1, 'from the first batch on')):
                h_, d_ = [r[j] for r in rates['host']], [r[j] for r in rates['device']]
                emit(what='GpuDetectionLoader, batches / s, ' + what, workers=workers, B=LB, batches=a.epoch_frames // LB, seg_mcus=seg,
                     host_median=round(float(np.median(h_)), 3), device_median=round(float(np.median(d_)), 3),
                     host_min=round(min(h_), 3), host_max=round(max(h_), 3), device_min=round(min(d_), 3), device_max=round(max(d_), 3),
                     device_above_host_by_more_than_the_host_spread=bool(np.median(d_) - np.median(h_) > max(h_) - min(h_)))


if __name__ == '__main__':
    main()
