"""Cost of the device JPEG encode (csrc/jpeg_encode.hip, utils/jpeg_encode.py) beside what it replaces, on one GPU.

The frames are those tools/bench_two_stage.py --pipeline feeds (8 cameras of 1080 x 1920, blocks of 16 x 16 pixels) with the
overlays `FramePipeline(draw=DrawStyle())` draws on them; quality 90, 4:2:0.  One JSON line per measurement:
  1. device-event time of one `t3d_jpeg_encode_u8` call over B = 1 and B = 8 frames (5 warm-up calls, then --reps timed:
     median, min, max) for seg_mcus in 1, 2, 4, 8, 16; the files are compared with Pillow's;
  2. beside it, in the same process: the device-to-host copy of the B raw frames into pinned memory, Pillow's `save` of the same
     frames on one core, and `t3d_jpeg_decode_u8` over the files just produced (the sibling kernel chain: the yardstick for
     whether the encoder's time is plausible);
  3. `FramePipeline(..., draw=DrawStyle())` at 1 and 8 cameras in three modes, wall clock per camera frame: frames left on the
     device; frames read back raw and encoded by Pillow; frames encoded on the device and only the bytes read back
     (`JpegEncoder.encode`).
`--encode-only SEG` runs only 5 + --reps encode calls of 8 frames at one seg_mcus: the run to put under
`rocprofv3 --kernel-trace --stats` for the time of each launch.
Usage: python tools/time_jpeg_encode.py [--reps 50] [--frames 120] [--parts encode,beside,pipeline] [--encode-only SEG]
       [--out FILE]  (default profiles/jpeg_encode_times.jsonl, rewritten by a run)"""
import argparse
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, '3d-object-detection.pytorch_amd'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from time_jpeg_decode import Decode, stats, timed  # noqa: E402

H, W, Q = 1080, 1920, 90
SWEEP = (1, 2, 4, 8, 16)


def stages(dtype=torch.bfloat16):
    """Detector, regressor model and the 8 camera frames of tools/bench_two_stage.py --pipeline."""
    from torchdet3d.builders import build_model
    from torchdet3d.models.ssd import SSD300
    from torchdet3d.utils import AttrDict, Detector
    cfg = AttrDict(dict(model=dict(name='mobilenetv2', num_classes=9, pretrained=False, storage_dtype='bf16', eval_storage_dtype='bf16')))
    model = build_model(cfg, export_mode=True).to('cuda')
    model.eval()
    det = Detector(SSD300('cuda', dtype), conf=0.0)
    gd = torch.Generator().manual_seed(0)
    sd = det.model.state_dict()
    for k in sd:                      # trained-looking BatchNorm buffers and biases: the scores must tell the anchors apart
        if k.startswith('bbox_head') and k.endswith('running_mean'):
            sd[k] = torch.randn(sd[k].shape, generator=gd) * 0.1
        elif k.startswith('bbox_head') and k.endswith('running_var'):
            sd[k] = torch.rand(sd[k].shape, generator=gd) + 0.5
        elif k.startswith('bbox_head.cls_convs') and k.endswith('.3.bias'):
            sd[k] = torch.randn(sd[k].shape, generator=gd) * 2.0
        elif k.startswith('bbox_head.reg_convs') and k.endswith('.3.bias'):
            sd[k] = torch.randn(sd[k].shape, generator=gd) * 0.5
    det.model.load_state_dict(sd)
    rng = np.random.default_rng(0)
    coarse = rng.integers(0, 256, (8, -(-H // 16), W // 16, 3), dtype=np.uint8)
    cams = torch.from_numpy(np.ascontiguousarray(coarse.repeat(16, 1).repeat(16, 2)[:, :H])).cuda()
    img, _ = det._enqueue(cams[0])
    sc = np.sort(det.model.detect(img)[0][:, 4])[::-1]
    cuts = [i for i in range(1, len(sc)) if sc[i - 1] > sc[i]]
    cut = min(cuts, key=lambda i: abs(i - 16))
    det.confidence = float((np.float64(sc[cut - 1]) + np.float64(sc[cut])) / 2)
    return det, model, cams


def pipeline(det, model, S, D=16):
    from torchdet3d.utils import DrawStyle, FramePipeline, IOUTracker, Regressor
    return FramePipeline(det, Regressor(model, (224, 224), max_detections=S * D), IOUTracker(device='cuda', streams=S, max_detections=D),
                         draw=DrawStyle())


def pillow_save(frame):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(frame).save(b, format='JPEG', quality=Q, subsampling=2)
    return b.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--frames', type=int, default=120, help='camera frames per figure of the pipeline part')
    ap.add_argument('--parts', default='encode,beside,pipeline')
    ap.add_argument('--encode-only', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jpeg_encode_times.jsonl'), help='the raw lines (rewritten by a run)')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    from torchdet3d.dataloaders.jpeg import DEFAULT_SEG_MCUS
    from torchdet3d.utils import JpegEncoder
    from torchdet3d.utils.jpeg_encode import DEFAULT_ENC_SEG_MCUS

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')
    if a.out and not a.encode_only:
        open(a.out, 'w').close()
    det, model, cams = stages()
    drawn = cams.clone()
    pipe = pipeline(det, model, 8)
    for _ in range(8):
        pipe.process_device(drawn)                       # (draws in place)
    torch.cuda.synchronize()
    del pipe
    if a.encode_only:
        enc = JpegEncoder(H, W, Q, '420', max_frames=8, cap_bytes=1 << 21, seg_mcus=a.encode_only)
        timed(lambda: enc.encode_device(drawn), a.reps)
        return
    parts = a.parts.split(',')
    host = drawn.cpu().numpy()
    want = [pillow_save(f) for f in host]
    emit(what='the frames', frame=[H, W], quality=Q, sampling='4:2:0', jpeg_bytes_mean=int(np.mean([len(f) for f in want])),
         raw_bytes=H * W * 3)
    files = want
    if 'encode' in parts:
        best = {}
        for B in (1, 8):
            for seg in SWEEP:
                enc = JpegEncoder(H, W, Q, '420', max_frames=B, cap_bytes=1 << 21, seg_mcus=seg)
                ms = timed(lambda: enc.encode_device(drawn[:B]), a.reps)
                got = enc.encode(drawn[:B])
                emit(what='t3d_jpeg_encode_u8, one call', B=B, seg_mcus=seg, equals_pillow=got == want[:B], **stats(ms))
                if B not in best or np.median(ms) < best[B][1]:
                    best[B] = (seg, float(np.median(ms)), max(ms) - min(ms))
                del enc
            emit(what='best seg_mcus of the sweep', B=B, seg_mcus=best[B][0], median_us=round(best[B][1] * 1e3, 1),
                 spread_us=round(best[B][2] * 1e3, 1), default=DEFAULT_ENC_SEG_MCUS)
    if 'beside' in parts:
        for B in (1, 8):
            pinned = torch.empty((B, H, W, 3), dtype=torch.uint8).pin_memory()
            u = stats(timed(lambda: pinned.copy_(drawn[:B], non_blocking=True), a.reps))
            emit(what='device-to-host copy of the raw frames into pinned memory', B=B, bytes=pinned.numel(),
                 GBps=round(pinned.numel() / (u['median_us'] * 1e-6) / 1e9, 1), **u)
            d = Decode(files[:B], DEFAULT_SEG_MCUS)
            ms = timed(d, a.reps)
            emit(what='t3d_jpeg_decode_u8 over the files just produced', B=B, seg_mcus=DEFAULT_SEG_MCUS, status_clean=not d.status.any().item(),
                 **stats(ms))
            del d, pinned
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < 3.0:
            pillow_save(host[n % 8])
            n += 1
        dt = time.perf_counter() - t0
        emit(what='Pillow save of one 1080x1920 frame, one core', frames_per_s=round(n / dt, 1), ms_per_frame=round(dt / n * 1e3, 2),
             ms_per_8_frames=round(8 * dt / n * 1e3, 1))
    if 'pipeline' not in parts:
        return
    for S in (1, 8):
        fr = cams[:S].clone()
        pipe = pipeline(det, model, S)
        enc = JpegEncoder(H, W, Q, '420', max_frames=S, cap_bytes=1 << 21)
        pinned = torch.empty((S, H, W, 3), dtype=torch.uint8).pin_memory()

        def on_device():
            pipe.process_device(fr)

        def raw_then_pillow():
            pipe.process_device(fr)
            pinned.copy_(fr)                              # (synchronises)
            return [pillow_save(f) for f in pinned.numpy()]

        def device_encode():
            pipe.process_device(fr)
            return enc.encode(fr)
        forms = {'frames_left_on_the_device': on_device, 'read_back_raw_and_pillow': raw_then_pillow, 'encoded_on_the_device': device_encode}
        for go in forms.values():
            for _ in range(6):
                go()
        torch.cuda.synchronize()
        ms = {k: [] for k in forms}
        for _ in range(3):
            for k, go in forms.items():
                iters = max(1, (a.frames if k != 'read_back_raw_and_pillow' else a.frames // 4) // S)
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(iters):
                    go()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t) / (iters * S) * 1e3)
        emit(what='FramePipeline with the draw stage, wall clock', cameras=S, replays=pipe.replays,
             jpeg_bytes_per_frame=int(np.mean([len(f) for f in device_encode()])),
             ms_per_camera_frame={k: {'median': round(float(np.median(v)), 4), 'min': round(min(v), 4), 'max': round(max(v), 4)}
                                  for k, v in ms.items()},
             camera_frames_per_s={k: round(1e3 / float(np.median(v)), 1) for k, v in ms.items()})
        del pipe, enc


if __name__ == '__main__':
    main()
