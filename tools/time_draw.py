"""The draw stage (t3d_draw_overlays_u8) at 1080 x 1920: HIP-event medians of the one launch for S in {1, 8} cameras with 0 and
16 objects per camera, beside a plain device copy of the same frames (what an out-of-place design would pay before it drew
anything), written to profiles/draw_overlay_bench.jsonl; then the frame time of the joined pipeline with the stage off and on
(tools/bench_two_stage.py --pipeline --draw, a process of its own -> profiles/pipeline_draw_bench.jsonl).
Usage: python tools/time_draw.py [--no-pipeline] [--launches 200]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, '3d-object-detection.pytorch_amd')]

import torch  # noqa: E402

from torchdet3d.utils import DrawStyle, draw_overlays  # noqa: E402

H, W, T = 1080, 1920, 16


def objects(S, rng):
    """16 boxes of 150..400 pixels per camera with a cabinet-projected cube inside each, tracked (ids >= 0) and labelled."""
    x0, y0 = rng.integers(0, W - 400, (S, T)), rng.integers(0, H - 400, (S, T))
    w, h = rng.integers(150, 400, (S, T)), rng.integers(150, 400, (S, T))
    boxes = np.stack([x0, y0, x0 + w, y0 + h], -1).astype(np.int32)
    kp = np.zeros((S, T, 9, 2))
    cx, cy, a, d = x0 + w / 2, y0 + h / 2, np.minimum(w, h) / 4, np.minimum(w, h) / 6
    kp[:, :, 0] = np.stack([cx, cy], -1)
    for i in range(8):
        sx, sy, sz = (i >> 2) & 1, (i >> 1) & 1, i & 1
        kp[:, :, i + 1] = np.stack([cx + (2 * sx - 1) * a + sz * d, cy + (2 * sy - 1) * a - sz * d / 2], -1)
    ids = rng.integers(0, 500, (S, T)).astype(np.int32)
    labels = rng.integers(0, 9, (S, T)).astype(np.int32)
    return [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (kp.reshape(S, T, 18), boxes, ids, labels)]


def median_us(fn, launches):
    for _ in range(10):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) for a, b in ev]) * 1e3
    return {'median': round(float(np.median(us)), 1), 'min': round(float(us.min()), 1), 'max': round(float(us.max()), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--no-pipeline', action='store_true')
    ap.add_argument('--launches', type=int, default=200)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    style = DrawStyle(draw_ids=True)
    lines = []
    for S in (1, 8):
        frames = torch.from_numpy(rng.integers(0, 256, (S, H, W, 3), dtype=np.uint8)).cuda()
        other = torch.empty_like(frames)
        kp, boxes, ids, labels = objects(S, rng)
        copy = median_us(lambda: other.copy_(frames), args.launches)
        for n in (0, T):
            count = torch.full((S,), n, dtype=torch.int32, device='cuda')
            us = median_us(lambda: draw_overlays(frames, kp, boxes=boxes, ids=ids, labels=labels, count=count, style=style), args.launches)
            line = {'metric': 't3d_draw_overlays_u8, one launch, HIP events around it (includes the event records)', 'cameras': S,
                    'frame': [H, W], 'objects_per_camera': n, 'launches': args.launches, 'draw_us': us, 'device_copy_of_the_frames_us': copy,
                    'frame_bytes': S * H * W * 3}
            lines.append(line)
            print(json.dumps(line), flush=True)
    out = os.path.join(ROOT, 'profiles', 'draw_overlay_bench.jsonl')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, 'w') as f:
        f.write(''.join(json.dumps(l) + '\n' for l in lines))
    if not args.no_pipeline:
        # a fresh process: the pipeline benchmark builds its own models
        subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'bench_two_stage.py'), '--pipeline', '--draw'], check=True)


if __name__ == '__main__':
    main()
