"""Cost of the device-resident detection loader (`data.cache = 'device'`: dataloaders/detection_arena.py, csrc/detect_draw.hip)
beside the loader it is an alternative to, on one GPU.  The frames, the folder, its two boxes an image and the train pipeline
are those of tools/time_jpeg_decode.py (generated 1440 x 1920, quality 90, 4:2:0).  One JSON line per measurement:
  fill  the arena's fill time and its bytes a frame (files, index, annotations);
  a.    `t3d_detect_draw` alone at B = --batch: device-event time of --reps calls (median, min, max), each with another batch
        key, beside the host's `boxes` + `records` on the same batches;
  b.    one arena batch on the device -- index_select, decode, draw, augment -- as device-event time, and the host time it
        takes to issue it (a. reports the longest crop search of its batches, in uniforms drawn);
  c.    frames / s of an epoch of --epoch-batches batches of --loader-batch from `ArenaDetectionLoader`, start-up included
        and from the first batch on, alternating with `GpuDetectionLoader` over `ObjectronFrames(decode='device')` at 2 and at
        16 workers on the same files, --alternations times; one line per epoch, then medians, ranges and the one condition:
        the arena's whole-epoch rate lies above the decode='device' loader's by more than that loader's min - max spread;
  d.    `DetectorTrainer.train` over the arena loader (frames / s of the epoch) beside the step time on one resident batch.
  crop  (not in the default list) `ArenaDetectionLoader(crop_decode=True)` beside the same loader with the flag off, per
        seg_mcus of --crop-seg-mcus: first the 5 + --reps timed keys give the same batches either way and the planner's diag
        gives the mean share of frame pixels and of 8x8 blocks it asked for; then --rounds rounds of device-event time of one
        arena batch, flag off and on alternating batch by batch (5 warm-up, --reps timed), median and min - max, and the
        condition: the flag-on median lies below the flag-off minimum; the verdict -- that condition in every round at the
        seg_mcus of the lowest flag-on median; then `DetectorTrainer.train` over --train-batches batches, off and on twice
        alternating, beside the step time on one resident batch.  (The flag-off path is the code before the flag existed:
        part b. with T3D_LIB set to a build of that library is the control.)
  crop_trace  5 + --reps batches with --crop-decode 0 or 1 at the first seg_mcus of --crop-seg-mcus and nothing timed: the run
        a kernel trace is taken of from outside (the whole-frame memset, entropy, IDCT, colour, planner, draw, augment).
Every part runs under its own time limit (SIGALRM in this one process; --limit seconds a part) and the tool stops at the first
failure or expired limit.
Usage: python tools/time_detection_arena.py [--batch 80] [--reps 50] [--alternations 5] [--epoch-batches 200]
       [--loader-batch 16] [--files 80] [--parts fill,a,b,c,d] [--limit 600] [--out FILE]
       [--crop-seg-mcus 1,2,4] [--rounds 3] [--train-batches 40] [--crop-decode 1]"""
import argparse
import contextlib
import json
import os
import signal
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-object-detection.pytorch_amd'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from time_jpeg_decode import TRAIN_PIPELINE, S, frame_jpeg, stats, write_dataset  # noqa: E402


@contextlib.contextmanager
def limit(seconds, what):
    def expired(*_):
        raise TimeoutError(f'{what}: not done after {seconds} s')
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(int(seconds))
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def epoch(loader, consume=None):
    """-> (batches, seconds of the whole epoch, seconds from the first batch on)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n, t1 = 0, None
    for batch in loader:
        if consume is not None:
            consume(batch)
        n += 1
        if t1 is None:
            torch.cuda.synchronize()
            t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return n, t2 - t0, t2 - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=80)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--alternations', type=int, default=5)
    ap.add_argument('--epoch-batches', type=int, default=200)
    ap.add_argument('--loader-batch', type=int, default=16)
    ap.add_argument('--files', type=int, default=80)
    ap.add_argument('--parts', default='fill,a,b,c,d')
    ap.add_argument('--limit', type=int, default=600)
    ap.add_argument('--crop-seg-mcus', default='1,2,4')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--train-batches', type=int, default=40)
    ap.add_argument('--crop-decode', type=int, default=1, choices=(0, 1))
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    from torchdet3d.dataloaders import DetectionAugmentPipeline, GpuDetectionLoader, ObjectronFrames
    from torchdet3d.dataloaders.detection_arena import ArenaDetectionLoader, DetectionArena
    parts = a.parts.split(',')

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')
    B, LB = a.batch, a.loader_batch
    files = [frame_jpeg(i) for i in range(a.files)]
    pipe = DetectionAugmentPipeline(TRAIN_PIPELINE, (S, S))
    with tempfile.TemporaryDirectory() as root:
        write_dataset(root, files, a.epoch_batches * LB)
        index = os.path.join(root, 'index.npy')

        def frames():
            ds = ObjectronFrames(root, 'train', decode='device')
            ds.build_index(index, threads=16)
            return ds
        with limit(a.limit, 'fill'):
            ds = frames()                                    # (builds and saves the index; not part of the fill time)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arena = DetectionArena(ds).fill()
            fill_s = time.perf_counter() - t0
            emit(what='DetectionArena: plan + fill', images=len(ds), distinct_files=len(files), seconds=round(fill_s, 3),
                 arena_bytes=arena.bytes, bytes_per_frame=round(arena.bytes / len(ds)), file_bytes_per_frame=round(float(arena.size.mean())),
                 G=arena.G)
        loader = ArenaDetectionLoader(arena, pipe, B, seed=3, prefetch=0)
        order = np.random.default_rng(0).permutation(len(ds))
        if 'a' in parts:
            with limit(a.limit, 'a'):
                from torchdet3d import _native as N
                from torchdet3d.dataloaders.detection_arena import key_words
                dev_ms, host_ms, longest = [], [], []
                for r in range(5 + a.reps):
                    idx = order[(r * B) % (len(ds) - B):][:B]
                    _, _, _, fr = loader.host_plan(idx)
                    d_fr = torch.from_numpy(fr).cuda()
                    G = arena.G
                    outs = [torch.empty(n, dtype=torch.uint8, device='cuda') for n in (B * 80, B * G * 16, B * G * 4, B * 4, B * 8)]
                    words = key_words((3, 0, 0, r))
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    N.call('t3d_detect_draw', loader._cfg.ctypes.data, len(loader._cfg), words.ctypes.data, len(words), N.ptr(d_fr), B,
                           N.ptr(arena.d_boxes), N.ptr(arena.d_labels), N.ptr(arena.d_box_start), len(arena), len(arena.labels), G,
                           *[N.ptr(o) for o in outs], N.stream())
                    e1.record()
                    e1.synchronize()
                    t0 = time.perf_counter()
                    prm = pipe.draw(B, (3, 0, 0, r))
                    pipe.boxes([ds._boxes[i] for i in idx], [ds._labels[i] for i in idx], fr[:, :3], prm)
                    rec = pipe.records(fr[:, :3], prm)
                    t1 = time.perf_counter()
                    if r >= 5:
                        dev_ms.append(e0.elapsed_time(e1))
                        host_ms.append((t1 - t0) * 1e3)
                        longest.append(int(outs[4].view(torch.int32).view(B, 2)[:, 1].max()))
                    assert outs[0].cpu().numpy().tobytes() == rec.tobytes(), 'the device records differ from the host\'s'
                emit(what='t3d_detect_draw alone', B=B, **stats(dev_ms), host_boxes_records=stats(host_ms, 1.0, 'ms'),
                     longest_search_uniforms_median=int(np.median(longest)), longest_search_uniforms_max=int(max(longest)),
                     records_equal_the_hosts=True)
        if 'b' in parts:
            with limit(a.limit, 'b'):
                dev_ms, host_ms = [], []
                for r in range(5 + a.reps):
                    idx = order[(r * B) % (len(ds) - B):][:B]
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    e0.record()
                    out = loader.finish(idx, (r,), prefetch=0)
                    e1.record()
                    t1 = time.perf_counter()
                    e1.synchronize()
                    if r >= 5:
                        dev_ms.append(e0.elapsed_time(e1))
                        host_ms.append((t1 - t0) * 1e3)
                    assert not loader.last_status.any().item()
                    del out
                emit(what='one arena batch on the device: index_select, decode, draw, augment', B=B, **stats(dev_ms, 1.0, 'ms'),
                     host_time_to_issue=stats(host_ms, 1.0, 'ms'))
        if 'c' in parts:
            rates = {}
            with limit(6 * a.limit, 'c'):
                for k in range(a.alternations):
                    for mode in ('arena', 'device, 2 workers', 'device, 16 workers'):
                        t0 = time.perf_counter()
                        if mode == 'arena':
                            ld = ArenaDetectionLoader(DetectionArena(frames()).fill(), pipe, LB, drop_last=True, seed=k)
                        else:
                            ld = GpuDetectionLoader(frames(), pipe, LB, shuffle=True, num_workers=int(mode.split()[1]), drop_last=True, seed=k)
                        setup = time.perf_counter() - t0
                        n, whole, rest = epoch(ld)
                        r = (n * LB / (whole + setup), n * LB / whole, (n - 1) * LB / rest)
                        rates.setdefault(mode, []).append(r)
                        emit(what='one epoch', loader=mode, B=LB, batches=n, alternation=k, seconds_to_build=round(setup, 3),
                             frames_per_s_build_and_epoch=round(r[0], 1), frames_per_s_whole_epoch=round(r[1], 1),
                             frames_per_s_after_the_first_batch=round(r[2], 1))
                        del ld
                        torch.cuda.empty_cache()
            for j, what in ((0, 'build (the arena: its fill) and whole epoch'), (1, 'whole epoch, start-up included'), (2, 'from the first batch on')):
                line = {}
                for mode, rs in rates.items():
                    v = [x[j] for x in rs]
                    line[mode] = dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))
                for mode in list(rates)[1:]:
                    spread = line[mode]['max'] - line[mode]['min']
                    line[f'arena above {mode} by more than its spread'] = bool(line['arena']['median'] - line[mode]['median'] > spread)
                emit(what='frames / s, ' + what, B=LB, batches=a.epoch_batches, **line)
        if 'd' in parts:
            with limit(a.limit, 'd'):
                from torchdet3d.models.ssd import SSD300
                from torchdet3d.trainer import DetectorTrainer
                tr = DetectorTrainer(SSD300(device='cuda:0', dtype=torch.bfloat16, seed=0), print_freq=1 << 30)
                ld = ArenaDetectionLoader(arena, pipe, B, drop_last=True, seed=1)
                batch = next(iter(ld))
                for _ in range(5):
                    tr.train_step(*batch[:4])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(20):
                    tr.train_step(*batch[:4])
                torch.cuda.synchronize()
                step_ms = (time.perf_counter() - t0) / 20 * 1e3
                n = len(ld)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.train(ld, 0)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                emit(what='DetectorTrainer.train over the arena loader', B=B, batches=n, ms_per_step_in_the_epoch=round(dt / n * 1e3, 3),
                     frames_per_s=round(n * B / dt, 1), ms_per_step_on_one_resident_batch=round(step_ms, 3),
                     frames_per_s_on_one_resident_batch=round(B / step_ms * 1e3, 1))
        if 'crop' in parts or 'crop_trace' in parts:
            segs = [int(s) for s in a.crop_seg_mcus.split(',')]

            def pair(seg):
                d = ObjectronFrames(root, 'train', decode='device')
                d.build_index(os.path.join(root, f'index_seg{seg}.npy'), threads=16, seg_mcus=seg)
                ar = DetectionArena(d).fill()
                return ar, [ArenaDetectionLoader(ar, pipe, B, seed=3, prefetch=0, crop_decode=flag) for flag in (False, True)]

            def one(ld, r):
                idx = order[(r * B) % (len(ds) - B):][:B]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = ld.finish(idx, (r,), prefetch=0)
                e1.record()
                e1.synchronize()
                assert not ld.last_status.any().item()
                return out, e0.elapsed_time(e1), idx
        if 'crop_trace' in parts:                   # (for a kernel trace from outside: 55 batches of one flag, nothing timed)
            with limit(a.limit, 'crop_trace'):
                _, lds = pair(segs[0])
                for r in range(5 + a.reps):
                    one(lds[a.crop_decode], r)
                emit(what='arena batches for a kernel trace', B=B, batches=5 + a.reps, seg_mcus=segs[0], crop_decode=bool(a.crop_decode))
        if 'crop' in parts:
            best, rounds_won = None, {}
            with limit(4 * a.limit, 'crop'):
                for seg in segs:
                    ar, (off, on) = pair(seg)
                    # the timed keys give the same batches either way; what the planner asked for, from its diag
                    px, bl = [], []
                    for r in range(5 + a.reps):
                        (want, _, idx), (got, _, _) = one(off, r), one(on, r)
                        assert all(torch.equal(u, v) for u, v in zip(got, want)), f'seg_mcus {seg}, batch {r}: the batches differ'
                        d = on.last_crop_diag.cpu().numpy().astype(np.float64)
                        px.append(float(np.mean(d[:, 0] / (ar.h[idx] * ar.w[idx]))))
                        bl.append(float(np.mean(d[:, 1] / ar.blocks[idx])))
                    emit(what='crop decode: the planner asked for', seg_mcus=seg, B=B, batches=5 + a.reps, batches_equal=True,
                         mean_share_of_frame_pixels=round(float(np.mean(px)), 4), mean_share_of_frame_blocks=round(float(np.mean(bl)), 4))
                    wins = []
                    for k in range(a.rounds):
                        ms = ([], [])
                        for r in range(5 + a.reps):              # flag off and on alternating, batch by batch, on the same key
                            for flag in (0, 1):
                                t = one((off, on)[flag], r)[1]
                                if r >= 5:
                                    ms[flag].append(t)
                        wins.append(bool(np.median(ms[1]) < min(ms[0])))
                        emit(what='one arena batch on the device, crop decode off / on', seg_mcus=seg, B=B, round=k, off=stats(ms[0], 1.0, 'ms'),
                             on=stats(ms[1], 1.0, 'ms'), on_median_below_off_min=wins[-1])
                        if best is None or np.median(ms[1]) < best[1]:
                            best = (seg, float(np.median(ms[1])))
                    rounds_won[seg] = wins
                    del ar, off, on
                    torch.cuda.empty_cache()
                emit(what='crop decode: verdict', best_seg_mcus=best[0], rule='on median below off min in every round, at the best seg_mcus',
                     gain=all(rounds_won[best[0]]), rounds=rounds_won[best[0]])
            with limit(a.limit, 'crop: train'):
                from torchdet3d.models.ssd import SSD300
                from torchdet3d.trainer import DetectorTrainer
                ar, _ = pair(best[0])
                walk = np.tile(order, -(-a.train_batches * B // len(order)))[:a.train_batches * B]
                line = {}
                for flag in (False, True, False, True):
                    tr = DetectorTrainer(SSD300(device='cuda:0', dtype=torch.bfloat16, seed=0), print_freq=1 << 30)
                    ld = ArenaDetectionLoader(ar, pipe, B, indices=walk, drop_last=True, seed=1, crop_decode=flag)
                    if 'resident' not in line:
                        batch = next(iter(ld))
                        for _ in range(5):
                            tr.train_step(*batch[:4])
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(20):
                            tr.train_step(*batch[:4])
                        torch.cuda.synchronize()
                        line['resident'] = round((time.perf_counter() - t0) / 20 * 1e3, 3)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    tr.train(ld, 0)
                    torch.cuda.synchronize()
                    line.setdefault('on' if flag else 'off', []).append(round((time.perf_counter() - t0) / len(ld) * 1e3, 3))
                    del tr, ld
                emit(what='DetectorTrainer.train over the arena loader, crop decode off / on', B=B, batches=a.train_batches, seg_mcus=best[0],
                     ms_per_step_off=line['off'], ms_per_step_on=line['on'], ms_per_step_on_one_resident_batch=line['resident'])


if __name__ == '__main__':
    try:
        main()
    except TimeoutError as e:
        print(json.dumps(dict(what='stopped', reason=str(e))), flush=True)
        sys.exit(124)
