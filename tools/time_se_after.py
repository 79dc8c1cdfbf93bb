"""Isolated timing of the one-launch gate-after-activation backward (t3d_se_after_bwd) against the three-launch sequence it
replaces (t3d_se_after_sums -> t3d_se_bwd_data -> t3d_se_after_apply), at the gated blocks of mobilenetv3_large_21k
(B = 256 @224^2).  Both paths live in the library, so they run in one process on one device, alternating.

Protocol: warm-up, then REPS repetitions of a LOOP-launch loop per path (device events around the loop); reported per path:
the median of the repetitions and their spread (max - min), in us per backward.  Verdict per shape = the engine's selection
rule: the one-launch kernel is used only where its median beats the sequence's by more than the larger of the two spreads.

usage: python tools/time_se_after.py [--dtype bf16|f32|both] [--batch 256] [--size 224] [--reps 7] [--loop 50] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, '3d-object-detection.pytorch_amd')]
import torch                                # noqa: E402
from torchdet3d import _native as N         # noqa: E402

# (C, R, stride of the gated plane, act, blocks of the model with this shape): HW = (crop side / stride)^2 -- 784, 784, 196, 196, 49, 49 @224^2
SHAPES = [(72, 24, 8, 'relu', 1), (120, 32, 8, 'relu', 2), (480, 120, 16, 'hswish', 1), (672, 168, 16, 'hswish', 1),
          (672, 168, 32, 'hswish', 1), (960, 240, 32, 'hswish', 2)]
NREP = 8


def loop_us(fn, loop):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(loop):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / loop * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtype', default='both')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--size', type=int, default=224, help='crop side (a multiple of 32)')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--loop', type=int, default=50)
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU: a timing taken anywhere else says nothing'
    assert args.reps >= 5
    B, rows = args.batch, []
    for name in (['bf16', 'f32'] if args.dtype == 'both' else [args.dtype]):
        tdt, dt = (torch.bfloat16, N.BF16) if name == 'bf16' else (torch.float32, N.F32)
        for C, R, stride, act, nblk in SHAPES:
            HW = (args.size // stride) ** 2
            g = torch.Generator(device='cuda').manual_seed(C + HW)
            rnd = lambda *s: torch.randn(*s, device='cuda', generator=g)
            y, dv = rnd(B * HW, C).to(tdt), (rnd(B * HW, C) * 0.1).to(tdt)
            scale, shift = torch.rand(C, device='cuda', generator=g) + 0.5, rnd(C) * 0.3
            w1, w2 = rnd(R, C) / C ** .5, rnd(C, R) / R ** .5
            pooled, h, q = rnd(B, C).abs(), rnd(B, R).clamp_min(0), rnd(B, C) * 2
            s = (q + 3).clamp(0, 6) / 6
            du = torch.empty_like(y)
            gg, dq, dp, ps = torch.empty(B, C, device='cuda'), torch.empty(B, C, device='cuda'), torch.empty(B, R, device='cuda'), \
                torch.empty(B, C, 2, device='cuda')
            ones, zeros = torch.ones(C, device='cuda'), torch.zeros(C, device='cuda')
            stats = torch.zeros(NREP, 2 * C, device='cuda', dtype=torch.float64)
            pro = N.prologue(scale, shift, None, act, False)
            st = N.stream()

            def fused():
                N.call('t3d_se_after_bwd', dt, N.ptr(dv), N.ptr(y), pro, N.ptr(w1), N.ptr(w2), N.ptr(h), N.ptr(q), N.ptr(s),
                       N.ptr(gg), N.ptr(dq), N.ptr(dp), N.ptr(du), N.ptr(stats), B, HW, C, R, st)

            def sequence():
                N.call('t3d_se_after_sums', dt, N.ptr(dv), N.ptr(y), pro, N.ptr(ps), B, HW, C, st)
                N.call('t3d_se_bwd_data', N.ptr(ps), N.ptr(pooled), N.ptr(zeros), N.ptr(ones), N.ptr(w1), N.ptr(w2), N.ptr(h),
                       N.ptr(q), N.ptr(s), N.ptr(gg), N.ptr(dq), N.ptr(dp), None, B, C, R, HW, st)
                N.call('t3d_se_after_apply', dt, N.ptr(dv), N.ptr(y), pro, N.ptr(s), N.ptr(gg), N.ptr(du), N.ptr(stats), B, HW, C, st)

            N.call('t3d_set_reduction_replicas', NREP, 2 * C)
            try:
                for fn in (fused, sequence):
                    loop_us(fn, 10)                                   # warm-up
                tf, ts = [], []
                for _ in range(args.reps):                            # alternating: both paths see the same neighbours
                    tf.append(loop_us(fused, args.loop))
                    ts.append(loop_us(sequence, args.loop))
            finally:
                N.call('t3d_set_reduction_replicas', 1, 0)
            mf, ms = statistics.median(tf), statistics.median(ts)
            sf, ss = max(tf) - min(tf), max(ts) - min(ts)
            win = ms - mf > max(sf, ss)
            nbytes = 2 * B * HW * C * y.element_size()               # dv + y, one pass
            rows.append(dict(dtype=name, B=B, C=C, R=R, HW=HW, act=act, blocks=nblk, fused_us=round(mf, 1),
                             fused_spread_us=round(sf, 1), sequence_us=round(ms, 1), sequence_spread_us=round(ss, 1),
                             plane_mb=round(nbytes / 1e6, 1), fused_selected=bool(win)))
            print(f'{name:4s} C={C:4d} R={R:3d} HW={HW:3d} x{nblk}: one launch {mf:7.1f} us (spread {sf:5.1f})   sequence {ms:7.1f} us '
                  f'(spread {ss:5.1f})   dv+y {nbytes / 1e6:6.1f} MB   -> {"ONE LAUNCH" if win else "sequence"}', flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
