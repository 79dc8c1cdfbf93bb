"""The Objectron evaluation stage at F = 256 frames, P = G = 8: HIP-event median of the two launches of
`ObjectronEvaluator.evaluate` (t3d_objectron_pairs + t3d_objectron_hitmiss), beside the wall time of the numpy restatement
(tests/objectron_eval_ref.py: per-frame / per-box / per-threshold loops, scipy hull per pair) for the same scene on this
machine's host.  Usage: python tools/time_objectron_eval.py"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, '3d-object-detection.pytorch_amd')]

import torch  # noqa: E402

import objectron_eval_ref as R  # noqa: E402
from torchdet3d.evaluation import ObjectronEvaluator  # noqa: E402

F, P, G = 256, 8, 8


def main():
    rng = np.random.default_rng(0)
    frames = []
    for _ in range(F):
        inst = [R.random_instance(rng) for _ in range(G)]
        frames.append(R.make_frame(inst, [i['kp2d'] + rng.normal(0, 0.005, (9, 2)) for i in inst]))
    d = {k: torch.from_numpy(v).cuda() for k, v in R.pack(frames, P, G).items()}
    ev = ObjectronEvaluator(F, P, G)

    def run():
        ev.reset()
        return ev.evaluate(d['pred'], d['pred_count'], d['kp2d'], d['kp3d'], d['vis'], d['gt_count'], d['planes'])

    for _ in range(5):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(30):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = np.array(ms)
    print(f'device: F={F} P={P} G={G}: both launches, HIP events: median {np.median(ms) * 1e3:.1f} us, '
          f'min {ms.min() * 1e3:.1f} us, max {ms.max() * 1e3:.1f} us over {len(ms)} runs', flush=True)
    res = ev.finalize()
    t0 = time.perf_counter()
    rows = R.evaluate_frames(frames)
    t1 = time.perf_counter()
    want = R.finalize(rows)
    print(f'numpy restatement, same scene, one host process: {t1 - t0:.2f} s for {F * P} boxes', flush=True)
    print('largest AP difference', max(np.abs(res['aps'][m] - want['aps'][m]).max() for m in R.METRICS),
          'matched', res['matched'], want['matched'])


if __name__ == '__main__':
    main()
