"""Regression stage of the two-stage pipeline (BASELINE config 5's second stage): detections of a 1080x1920 uint8 frame ->
crop + resize (t3d_crop_resize_u8) -> batched all-heads regression -> arg-max head, per frame.
usage: python tools/bench_two_stage.py [--model mobilenetv2] [--dets 16] [--frames 200] [--dtype bf16] [--detector] [--track] [--pipeline [--draw]]
Prints one JSON line: frames/s and crops/s with the frame resident in HBM, the same with the 6.2 MB H2D copy of every frame
inside the timed region, and the oracle's host crop+resize loop (numpy, 1 core) for the same detections.
--track adds the third stage (torchdet3d.utils.IOUTracker, t3d_track_step): the regression loop with the device tracker fed
from Regressor.regress (one frame per launch, and --batch-frames cameras per launch), the same loop with what a host tracker
needs instead (a D2H copy of rects and keypoints and a synchronisation per frame; the host tracker's own time not counted),
and the HIP-event time of t3d_track_step alone for 1 / 8 / 32 streams.
--pipeline times the joined three-stage loop instead (torchdet3d.utils.FramePipeline) and prints / appends one JSON line per
(cameras, cap) to profiles/pipeline_two_stage_bench.jsonl: S in {1, 8} cameras of 1080x1920 frames resident in HBM, cap D = 16
with the confidence set so that about 16 rows pass and D = 64 at the same confidence (what padding costs), three forms
alternated in one process, three repetitions each: (a) the host-joined chain per camera (Detector.get_detections ->
Regressor.get_detections -> IOUTracker.process -> get_tracked_objects -> transform_kp), (b) the pipeline launch by launch,
(c) the pipeline replayed from its recorded plan.
--draw (with --pipeline) adds (d) / (e): forms (b) / (c) with the draw stage as the chain's last launch (FramePipeline(draw=DrawStyle()),
on a copy of the frames of their own: the overlays stay on it from frame to frame), at D = 16 only, and writes
profiles/pipeline_draw_bench.jsonl instead."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, '3d-object-detection.pytorch_amd')]
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument('--model', default='mobilenetv2')
ap.add_argument('--dets', type=int, default=16)
ap.add_argument('--frames', type=int, default=200)
ap.add_argument('--dtype', default='bf16')
ap.add_argument('--batch-frames', type=int, nargs='*', default=[8, 32], help='with --detector: frames per launch chain of the '
                'batched detector stage (Detector.get_detections_batch; BASELINE config 5 says "batched on 1 MI355X")')
ap.add_argument('--detector', action='store_true', help='time the whole pipeline: SSD300-MobileNetV2 detector (models/ssd.py) '
                'on the frame, then the regression stage on its detections (scripts/demo.py:48-90)')
ap.add_argument('--track', action='store_true', help='add the tracking stage: device tracker fed from Regressor.regress, against '
                'no tracking and against the per-frame D2H copy + sync a host tracker needs; t3d_track_step alone for 1 / 8 / 32 streams')
ap.add_argument('--pipeline', action='store_true', help='time the joined detector -> regressor -> tracker -> frame-pixel keypoints '
                'loop: host-joined chain against FramePipeline launch by launch and replayed; S in {1, 8}, D in {16, 64}')
ap.add_argument('--draw', action='store_true', help='with --pipeline: also time the pipeline with the draw stage (boxes, keypoints and '
                'labels drawn on the frames in place) launch by launch and replayed')
args = ap.parse_args()

from torchdet3d.builders import build_model
from torchdet3d.utils import AttrDict, Regressor

cfg = AttrDict(dict(model=dict(name=args.model, num_classes=9, pretrained=False, storage_dtype=args.dtype,
                               eval_storage_dtype=args.dtype)))      # inference in the SAME storage precision (opt-in for bf16)
model = build_model(cfg, export_mode=True).to('cuda')
model.eval()
H, W, n = 1080, 1920, args.dets


def bench_pipeline():
    from torchdet3d.models.ssd import SSD300
    from torchdet3d.utils import Detector, FramePipeline, IOUTracker
    det = Detector(SSD300('cuda', torch.bfloat16 if args.dtype == 'bf16' else torch.float32), conf=0.0)
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
    # blocks of 16 x 16 pixels: structure that survives the resize to 300 x 300 (white noise averages to one grey for every anchor)
    coarse = rng.integers(0, 256, (8, -(-H // 16), W // 16, 3), dtype=np.uint8)
    cams = torch.from_numpy(np.ascontiguousarray(coarse.repeat(16, 1).repeat(16, 2)[:, :H])).cuda()
    img, _ = det._enqueue(cams[0])
    sc = np.sort(det.model.detect(img)[0][:, 4])[::-1]
    cuts = [i for i in range(1, len(sc)) if sc[i - 1] > sc[i]]                      # (equal scores cannot be split)
    cut = min(cuts, key=lambda i: abs(i - 16))
    det.confidence = float((np.float64(sc[cut - 1]) + np.float64(sc[cut])) / 2)     # `cut` rows of camera 0 pass: 16, or the nearest
    frames_per_figure = max(args.frames, 200)
    out_path = os.path.join(ROOT, 'profiles', 'pipeline_draw_bench.jsonl' if args.draw else 'pipeline_two_stage_bench.jsonl')
    lines = []
    for S in (1, 8):
        fr = cams[:S].contiguous()
        iters = -(-frames_per_figure // S)
        for D in ((16,) if args.draw else (16, 64)):
            reg = Regressor(model, (224, 224), max_detections=S * D)
            solo = [IOUTracker(device='cuda', max_detections=D) for _ in range(S)]
            os.environ['T3D_STEP_PLAN'] = '0'
            direct = FramePipeline(det, reg, IOUTracker(device='cuda', streams=S, max_detections=D))
            os.environ.pop('T3D_STEP_PLAN')
            replayed = FramePipeline(det, reg, IOUTracker(device='cuda', streams=S, max_detections=D))
            passed = []

            def host_chain(k):
                for _ in range(k):
                    for s in range(S):
                        dets = det.get_detections(fr[s])[:D]
                        outs = reg.get_detections(fr[s], dets)
                        solo[s].process(fr[s], dets, [o[0].reshape(-1) for o in outs])
                        objs = solo[s].get_tracked_objects()
                        [Regressor.transform_kp(np.array(o.kp).reshape(9, 2), o.rect[:4]) for o in objs]
                        passed.append(len(dets))

            def device_chain(pipe):
                def go(k):
                    for _ in range(k):
                        pipe.process_device(fr)
                return go

            def host_lists(pipe):
                def go(k):
                    for _ in range(k):
                        pipe.process(fr[0])
                return go
            forms = {'a_host_joined': host_chain, 'b_launch_by_launch': device_chain(direct), 'c_replayed': device_chain(replayed)}
            if args.draw:
                from torchdet3d.utils import DrawStyle
                fr_draw = fr.clone()
                os.environ['T3D_STEP_PLAN'] = '0'
                direct_draw = FramePipeline(det, reg, IOUTracker(device='cuda', streams=S, max_detections=D), draw=DrawStyle())
                os.environ.pop('T3D_STEP_PLAN')
                replayed_draw = FramePipeline(det, reg, IOUTracker(device='cuda', streams=S, max_detections=D), draw=DrawStyle())

                def draw_chain(pipe):
                    def go(k):
                        for _ in range(k):
                            pipe.process_device(fr_draw)
                    return go
                forms.update(d_launch_by_launch_draw=draw_chain(direct_draw), e_replayed_draw=draw_chain(replayed_draw))
            if S == 1:      # the demo's four host lists per frame: one read-back and one synchronisation each
                forms.update(b_launch_by_launch_host_lists=host_lists(direct), c_replayed_host_lists=host_lists(replayed))
            for go in forms.values():                                  # warm-up of every form at this shape (records the plan)
                go(6)
            torch.cuda.synchronize()
            assert replayed.replays > 0 and direct.replays == 0
            assert not args.draw or (replayed_draw.replays > 0 and direct_draw.replays == 0)
            ms = {k: [] for k in forms}
            for _ in range(3):
                for k, go in forms.items():
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    go(iters)
                    torch.cuda.synchronize()
                    ms[k].append((time.perf_counter() - t) / (iters * S) * 1e3)
            res = replayed.process_device(fr)
            line = {'metric': 'joined detector -> regressor -> tracker -> frame-pixel keypoints, 1080x1920 frames in HBM', 'cameras': S,
                    'cap_D': D, 'model': args.model, 'dtype': args.dtype, 'camera_frames_per_figure': iters * S, 'conf': round(det.confidence, 6),
                    'rows_passing_per_camera': res['counts'].tolist(), 'overflow_per_camera': res['overflow'].tolist(),
                    'host_chain_detections_per_camera_frame': round(float(np.mean(passed)), 2),
                    'ms_per_camera_frame': {k: {'median': round(float(np.median(v)), 4), 'min': round(min(v), 4), 'max': round(max(v), 4),
                                                'runs': [round(x, 4) for x in v]} for k, v in ms.items()},
                    'camera_frames_per_s': {k: round(1e3 / float(np.median(v)), 1) for k, v in ms.items()}}
            lines.append(line)
            print(json.dumps(line), flush=True)
            del direct, replayed
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(''.join(json.dumps(l) + '\n' for l in lines))


if args.pipeline:
    from torchdet3d.utils import Regressor as _R      # noqa: F401
    bench_pipeline()
    sys.exit(0)
rng = np.random.default_rng(0)
frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
x0 = rng.integers(0, W - 400, n); y0 = rng.integers(0, H - 400, n)
rects = np.stack([x0, y0, x0 + rng.integers(60, 400, n), y0 + rng.integers(60, 400, n)], 1).astype(np.int32)
reg = Regressor(model, (224, 224), max_detections=n)
fd, rd = torch.from_numpy(frame).cuda(), torch.from_numpy(rects).cuda()
fh = torch.from_numpy(frame).pin_memory()


def run(frames, upload):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(frames):
        f = fd
        if upload:
            fd.copy_(fh, non_blocking=True)
        kp, labels = reg.regress(f, rd)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / frames


run(20, False)
t_res, t_up = run(args.frames, False), run(args.frames, True)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(50):
    reg.crop_resize(fd, rd)
e1.record(); torch.cuda.synchronize()
t_crop = e0.elapsed_time(e1) / 50 * 1e-3
from oracle.crop_resize import crop, resize_linear_u8      # cpu_baseline leg only
t = time.perf_counter()
for r in rects:
    resize_linear_u8(crop(frame, r), (224, 224))
t_cpu = time.perf_counter() - t
extra = {}
if args.detector:
    from torchdet3d.models.ssd import SSD300
    from torchdet3d.utils import Detector
    det = Detector(SSD300('cuda', torch.bfloat16 if args.dtype == 'bf16' else torch.float32), conf=0.3)
    gd = torch.Generator().manual_seed(0)
    sd = det.model.state_dict()
    for k in sd:
        if k.startswith('bbox_head.cls_convs') and k.endswith('.3.bias'):
            sd[k] = torch.randn(sd[k].shape, generator=gd) * 2.0
    det.model.load_state_dict(sd)

    def pipeline(frames):
        torch.cuda.synchronize()
        t = time.perf_counter()
        nd = 0
        for _ in range(frames):
            dets = det.get_detections(fd)[:n]
            nd += len(dets)
            if dets:
                reg.get_detections(fd, dets)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / frames, nd / frames

    def detector_only(frames):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(frames):
            det.get_detections(fd)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / frames
    def detector_batched(fb, reps):
        stack = fd.unsqueeze(0).repeat(fb, 1, 1, 1).contiguous()
        det.get_detections_batch(stack)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            out = det.get_detections_batch(stack)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / (reps * fb), out

    def pipeline_batched(fb, reps):
        # detector over fb frames in one chain, then the regression stage frame by frame on its detections
        stack = fd.unsqueeze(0).repeat(fb, 1, 1, 1).contiguous()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            for f, dets in enumerate(det.get_detections_batch(stack)):
                if dets:
                    reg.get_detections(stack[f], dets[:n])
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / (reps * fb)
    pipeline(5)
    tp, nd = pipeline(max(20, args.frames // 4))
    td = detector_only(max(20, args.frames // 4))
    batched = {}
    one = det.get_detections(fd)
    for fb in args.batch_frames:
        tb, outb = detector_batched(fb, max(5, args.frames // (4 * fb)))
        assert all(o == one for o in outb), 'batched detections differ from the one-frame path'
        tpb = pipeline_batched(fb, max(3, args.frames // (8 * fb)))
        batched[str(fb)] = {'detector_ms_per_frame': round(tb * 1e3, 3), 'detector_frames_per_s': round(1 / tb, 1),
                            'pipeline_ms_per_frame': round(tpb * 1e3, 3), 'pipeline_frames_per_s': round(1 / tpb, 1)}
    extra = {'pipeline_ms_per_frame': round(tp * 1e3, 3), 'pipeline_frames_per_s': round(1 / tp, 1), 'detections_regressed_per_frame': round(nd, 1),
             'detector_ms_per_frame': round(td * 1e3, 3), 'batched_frames_per_launch_chain': batched, 'detector': 'SSD300-MobileNetV2 (random weights), one frame per launch chain, host read-back of the detections'}
if args.track:
    from torchdet3d.utils import IOUTracker

    def track_loop(frames, mode):
        tr = IOUTracker(device='cuda', max_detections=n) if mode == 'device' else None
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(frames):
            kp, labels = reg.regress(fd, rd)
            if mode == 'device':
                tr.process_device(rd, kp)
            elif mode == 'host':
                rd.cpu(), kp.cpu()              # what a host tracker needs every frame: both copies, each waits for the stream
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / frames

    def track_loop_batched(fb, reps, track):
        # fb cameras: the regression stage frame by frame, then ONE tracker launch for the fb streams
        tr = IOUTracker(device='cuda', streams=fb, max_detections=n)
        rb, kb = rd.unsqueeze(0).repeat(fb, 1, 1).contiguous(), torch.zeros(fb, n, 18, device='cuda')
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            for f in range(fb):
                kp, labels = reg.regress(fd, rd)
                if track:
                    kb[f].copy_(kp.view(n, 18))
            if track:
                tr.process_batch_device(rb, kb)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / (reps * fb)

    def step_alone(S, launches=200, dets=16):
        # `dets` objects per stream, jittered by a few pixels from frame to frame: every detection continues its track
        g = np.random.default_rng(1)
        bx = g.integers(0, W - 400, (S, dets, 1)); by = g.integers(0, H - 400, (S, dets, 1))
        base = np.concatenate([bx, by, bx + g.integers(90, 320, (S, dets, 1)), by + g.integers(90, 320, (S, dets, 1))], 2)
        variants = [torch.from_numpy((base + g.integers(-3, 4, base.shape)).astype(np.int32)).cuda() for _ in range(8)]
        kv = [torch.from_numpy((0.5 + g.normal(0, 0.01, (S, dets, 18))).astype(np.float32)).cuda() for _ in range(8)]
        tr = IOUTracker(device='cuda', streams=S, max_detections=dets)
        for i in range(16):
            tr.process_batch_device(variants[i % 8], kv[i % 8])
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(ev):
            a.record()
            tr.process_batch_device(variants[i % 8], kv[i % 8])
            b.record()
        torch.cuda.synchronize()
        single = float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3
        a, b = ev[0]
        a.record()
        for i in range(launches):
            tr.process_batch_device(variants[i % 8], kv[i % 8])
        b.record()
        torch.cuda.synchronize()
        nt = tr.num_tracks
        return {'event_pair_median_us': round(single, 1), 'back_to_back_us': round(a.elapsed_time(b) / launches * 1e3, 1),
                'tracks_per_stream': nt if isinstance(nt, int) else int(np.mean(nt))}

    nf = args.frames
    track_loop(20, 'device')
    t_none, t_dev, t_host = track_loop(nf, None), track_loop(nf, 'device'), track_loop(nf, 'host')
    tb = {}
    for fb in args.batch_frames:
        reps = max(3, nf // fb)
        track_loop_batched(fb, 2, True)
        a, b = track_loop_batched(fb, reps, False), track_loop_batched(fb, reps, True)
        tb[str(fb)] = {'frames_per_s_no_tracking': round(1 / a, 1), 'frames_per_s_device_tracker': round(1 / b, 1)}
    extra['tracking'] = {
        'frames_per_s_no_tracking': round(1 / t_none, 1), 'frames_per_s_device_tracker': round(1 / t_dev, 1),
        'frames_per_s_host_tracker_copies': round(1 / t_host, 1), 'ms_per_frame_no_tracking': round(t_none * 1e3, 3),
        'ms_per_frame_device_tracker': round(t_dev * 1e3, 3), 'ms_per_frame_host_tracker_copies': round(t_host * 1e3, 3),
        'cameras_per_tracker_launch': tb,
        't3d_track_step_alone_16_dets': {str(S): step_alone(S) for S in (1, 8, 32)},
        'what': 'regression loop + IOUTracker.process_device per frame; host_tracker_copies = D2H of rects and keypoints with '
                'a synchronisation per frame (the host tracker itself not counted); step alone: HIP events around one launch '
                '(includes the event records) and 200 launches back to back'}
print(json.dumps({**extra, 'metric': f'two-stage regression stage, {n} detections per 1080x1920 frame, {args.model}', 'frames_per_s': round(1 / t_res, 1),
                  'crops_per_s': round(n / t_res, 1), 'ms_per_frame': round(t_res * 1e3, 3), 'frames_per_s_with_h2d': round(1 / t_up, 1),
                  'crop_resize_us': round(t_crop * 1e6, 1), 'dtype': args.dtype,
                  'cpu_baseline': {'what': 'oracle crop + 8-bit bilinear resize loop (numpy), 1 core', 'ms_per_frame': round(t_cpu * 1e3, 2)}}))
