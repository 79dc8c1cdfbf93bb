"""The detector's COCO bbox evaluation at the config's batch (B = 80 = samples_per_gpu, G = 8): HIP-event medians of
`SSD300.detect_device` alone (random frames through an untrained detector) and of the two evaluation launches
(t3d_ssd_cap_per_image + t3d_coco_match through `DetectionEvaluator.evaluate_detections`) on detections decoded from random
head outputs as tools/time_ssd_loss.py makes them (the 2044 real anchors, bf16, the head's padded rows); host wall-clock of
`finalize` over a record of 4000 images (the read-back and the numpy accumulation apart) and of the plain-loop restatement of
the per-image matching (tests/coco_eval_ref.py) on the same batch.  Appends the raw lines to
profiles/detection_eval_times.jsonl.
Usage: python tools/time_detection_eval.py [--out profiles/detection_eval_times.jsonl]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, '3d-object-detection.pytorch_amd')]

import torch  # noqa: E402

import coco_eval_ref as C  # noqa: E402
import ssd_loss_ref as R  # noqa: E402
from time_ssd_loss import B, CLS_STRIDES, G, HWS, NAS, NC, REG_STRIDES, median_ms  # noqa: E402
from torchdet3d import _native as N  # noqa: E402
from torchdet3d.evaluation import DetectionEvaluator  # noqa: E402
from torchdet3d.evaluation import detection_eval as E  # noqa: E402
from torchdet3d.models.ssd import INPUT_SIZE, STDS, SSD300  # noqa: E402

IMAGES, K = 4000, 200


def decode(outs, anchors, dev):
    """t3d_ssd_decode_nms over random head outputs, as `SSD300.detect_device` calls it."""
    nl = len(outs)
    out = torch.zeros(B, NC, K, 6, device=dev)
    cnt = torch.zeros(B, NC, dtype=torch.int32, device=dev)
    P, I = ctypes.c_void_p * nl, ctypes.c_int * nl
    host = (P(*[o[0].data_ptr() for o in outs]), P(*[o[1].data_ptr() for o in outs]), I(*HWS), I(*NAS), I(*CLS_STRIDES), I(*REG_STRIDES))
    stds = (ctypes.c_float * 4)(*STDS)
    N.call('t3d_ssd_decode_nms', N.BF16, nl, *[ctypes.addressof(h) for h in host], N.ptr(anchors), B, NC, 0.02, 0.45, K,
           float(INPUT_SIZE), float(INPUT_SIZE), ctypes.addressof(stds), N.ptr(out), N.ptr(cnt), N.stream())
    torch.cuda.synchronize()
    return out, cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'detection_eval_times.jsonl'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the timing needs the GPU'
    rng = np.random.default_rng(0)
    dev, A = 'cuda:0', 2044
    cls = (rng.standard_normal((B, A, NC + 1)) * 2).astype(np.float32)
    reg = rng.standard_normal((B, A, 4)).astype(np.float32)
    gb, gl = R._random_gt(rng, B, G)
    gc = rng.integers(1, G + 1, B).astype(np.int32)
    shapes = np.tile(np.array([[1440, 1920]], np.int32), (B, 1))
    anchors = torch.from_numpy(R.real_anchors()).to(dev)
    outs = [(torch.from_numpy(c).to(dev).to(torch.bfloat16), torch.from_numpy(r).to(dev).to(torch.bfloat16), hw)
            for c, r, hw in zip(R.to_levels(cls, HWS, NAS, NC + 1, CLS_STRIDES, pad=0.0), R.to_levels(reg, HWS, NAS, 4, REG_STRIDES, pad=0.0), HWS)]
    out, cnt = decode(outs, anchors, dev)
    gt = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (gb, gl, gc, shapes)]
    common = dict(B=B, G=G, num_classes=NC, max_per_class=K, device=torch.cuda.get_device_name(0))
    rows = []

    def row(**kw):
        rows.append(dict(kw, **common))
        print(json.dumps(rows[-1]), flush=True)

    # ---- detect_device alone
    det = SSD300(device=dev, dtype=torch.bfloat16)
    imgs = torch.from_numpy(rng.integers(0, 256, (B, INPUT_SIZE, INPUT_SIZE, 3), dtype=np.uint8)).to(dev)
    med, lo, hi, n = median_ms(lambda: det.detect_device(imgs))
    row(what='detect_device', median_us=round(med * 1e3, 1), min_us=round(lo * 1e3, 1), max_us=round(hi * 1e3, 1), runs=n,
        timer='HIP events around the call', input='random uint8 frames, untrained SSD300, bf16')

    # ---- the two evaluation launches
    ev = DetectionEvaluator(det, IMAGES)

    def launches():
        ev.base = 0
        ev.evaluate_detections(out, cnt, *gt)
    med, lo, hi, n = median_ms(launches)
    ndt = ev.record()['ndt']
    row(what='t3d_ssd_cap_per_image + t3d_coco_match', median_us=round(med * 1e3, 1), min_us=round(lo * 1e3, 1),
        max_us=round(hi * 1e3, 1), runs=n, timer='HIP events around evaluate_detections',
        input='detections decoded from random head outputs (time_ssd_loss.py), ori_shape 1440 x 1920',
        detections_before_cap=int(cnt.sum().item()), detections_matched_against=int(ndt.sum()))

    # ---- finalize over 4000 images: the same batch 50 times
    ev.reset()
    for _ in range(IMAGES // B):
        ev.evaluate_detections(out, cnt, *gt)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = ev.record()
    t1 = time.perf_counter()
    precision, recall = E.accumulate(*[h[k] for k in ('score', 'dtm', 'dtig', 'ndt', 'ngt', 'valid')])
    stats = E.summarize(precision, recall)
    t2 = time.perf_counter()
    ev._result = None
    res = ev.finalize()
    t3 = time.perf_counter()
    assert np.array_equal(res['stats'], stats)
    row(what='finalize', images=IMAGES, total_ms=round((t3 - t2) * 1e3, 1), readback_ms=round((t1 - t0) * 1e3, 1),
        accumulate_summarize_ms=round((t2 - t1) * 1e3, 1), record_bytes=int(sum(v.nbytes for v in h.values())),
        timer='host wall clock, one run', bbox_mAP=res['bbox_mAP'])

    # ---- the plain-loop restatement of the per-image half on the same batch
    t0 = time.perf_counter()
    want, _ = C.record_of(out.cpu().numpy(), cnt.cpu().numpy(), gb, gl, gc, shapes, INPUT_SIZE, INPUT_SIZE, det.max_per_img)
    t1 = time.perf_counter()
    equal = all(np.array_equal(h[k][:B], want[k]) for k in want)
    row(what='numpy restatement of cap + match (tests/coco_eval_ref.py)', total_ms=round((t1 - t0) * 1e3, 1),
        timer='host wall clock, one run, one core', record_equal_to_device=bool(equal))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        for r in rows:
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
