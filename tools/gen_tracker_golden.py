"""Records tests/golden/tracker.npz from the REFERENCE's own IOUTracker.
usage: python tools/gen_tracker_golden.py --reference /path/to/reference/checkout [--out tests/golden/tracker.npz]

The reference's torchdet3d/utils/tracking_tools.py needs only numpy and scipy, so it is loaded by file path (its package
would pull in cv2).  Synthetic scenes (tests/tracker_ref.py::make_scene) run through it under four parameter sets on four
seeds each; per frame the file keeps the inputs, the `get_tracked_objects()` result (rect[:4], keypoints as float64, id),
`len(tracker.tracks)` and `last_global_id` -- inputs, parameters and recorded results only.

The reference is instrumented from outside (wrappers around `linear_sum_assignment`, `_iou`, `_filter_last_3d_box` and
`global_id_getter`) to measure how far every branch decision is from flipping; a seed is used only if all of these margins
are >= 1e-4, so that an fp64 restatement of the float32 / float64 mix of the reference cannot take another branch:
  * assigned cost vs match_threshold, IoU vs track_detection_iou_thresh, mean keypoint distance vs add_treshold,
  * the total of the second-best assignment (brute force over all assignments up to 8 columns; beyond, the
    best assignment without each optimal pair in turn) vs the best.
Over the whole file it asserts: a released id is reused, a track leaves through track_clear_thresh, frames with more and
with fewer detections than active tracks, and a frame without detections while tracks are live."""
import argparse
import importlib.util
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'tests')]
from tracker_ref import DEFAULTS, make_scene      # noqa: E402  (the scene recipe only)

SETS = {
    'defaults': {},
    'demo': dict(time_window=10, continue_time_thresh=5),
    'demo_align': dict(time_window=10, continue_time_thresh=5, align_kp=True),
    'tight': dict(time_window=3, continue_time_thresh=1, match_threshold=0.25, track_detection_iou_thresh=0.6,
                  no_updated_frames_treshold=2, track_clear_thresh=12),
}
MARGIN, SEEDS_PER_SET, FRAMES = 1e-4, 4, 48
_perms = {}


def second_best_gap(cost, best_total, solver):
    c = cost.astype(np.float64)
    if c.shape[0] > c.shape[1]:
        c = c.T
    n, m = c.shape
    if m > 8:                                     # too many to enumerate: any other assignment leaves out one optimal pair
        r, k = solver(c)
        gaps = []
        for i, j in zip(r, k):
            alt = c.copy()
            alt[i, j] = 1e6
            ar, ak = solver(alt)
            gaps.append(alt[ar, ak].sum() - best_total)
        return min(gaps)
    if (n, m) not in _perms:
        _perms[n, m] = np.array(list(itertools.permutations(range(m), n)), dtype=np.int64)
    totals = np.sort(c[np.arange(n), _perms[n, m]].sum(1))
    assert abs(totals[0] - best_total) < 1e-9, 'the reference did not return the optimum'
    return totals[1] - totals[0] if len(totals) > 1 else np.inf


def run_scene(mod, params, scene):
    """-> (recorded arrays, stats) of one scene on the reference."""
    stats = dict(cost=np.inf, iou=np.inf, kp=np.inf, gap=np.inf, skips=set(), max_matrix=(0, 0), more=False, fewer=False,
                 blank=False, reuse=False, cleared=0, nouf=0, last_global_id=0, max_live=0)
    tracker = mod.IOUTracker(**params)
    o_lsa, o_iou, o_filter = mod.linear_sum_assignment, mod.IOUTracker._iou, mod.Track._filter_last_3d_box

    def lsa(cost):
        r, c = o_lsa(cost)
        stats['max_matrix'] = max(stats['max_matrix'], cost.shape, key=lambda s: s[0] * s[1])
        stats['more'] |= cost.shape[0] > cost.shape[1]
        stats['fewer'] |= cost.shape[0] < cost.shape[1]
        stats['gap'] = min(stats['gap'], second_best_gap(cost, cost.astype(np.float64)[r, c].sum(), o_lsa))
        stats['cost'] = min(stats['cost'], np.abs(cost[r, c].astype(np.float64) - tracker.match_threshold).min())
        return r, c

    def iou(self, b1, b2, a1=None, a2=None):
        v = o_iou(self, b1, b2, a1, a2)
        stats['iou'] = min(stats['iou'], abs(v - tracker.track_detection_iou_thresh))
        return v

    def filt(self, filter_speed, add_treshold, no_updated_frames_treshold):
        if self.timestamps[-1] - self.timestamps[-2] == 1:
            saved = self.kps[-2], self.kps[-1]
            self.kps[-2] = np.array(self.kps[-2]).reshape(9, 2)
            self.kps[-1] = np.array(self.kps[-1]).reshape(9, 2)
            d = np.mean(np.linalg.norm(self.kps[-1].astype(np.float64) - self.kps[-2].astype(np.float64), axis=1))
            if self.align_kp:
                idx = self._align_kp_positions()
                after = np.mean(np.linalg.norm(self.kps[-1][idx].astype(np.float64) - self.kps[-2].astype(np.float64), axis=1))
                if idx != list(range(9)):
                    stats['kp'] = min(stats['kp'], abs(after - d))
                d = min(d, after)
            stats['kp'] = min(stats['kp'], abs(d - add_treshold))
            self.kps[-2], self.kps[-1] = saved
        o_filter(self, filter_speed, add_treshold, no_updated_frames_treshold)
        stats['nouf'] = max(stats['nouf'], self.no_updated_frames)

    o_getter = tracker.global_id_getter

    def getter():
        stats['reuse'] |= not tracker.global_ids_queue.empty()
        return o_getter()

    mod.linear_sum_assignment, mod.IOUTracker._iou, mod.Track._filter_last_3d_box = lsa, iou, filt
    tracker.global_id_getter = getter
    rec = dict(det_boxes=[], det_kps=[], det_counts=[], out_boxes=[], out_kps=[], out_ids=[], out_counts=[], num_tracks=[],
               last_global_id=[])
    try:
        for boxes, kps in scene:
            detections = [(int(b[0]), int(b[1]), int(b[2]), int(b[3]), 0.9, 0) for b in boxes]   # the detector's 6-tuples
            ends = {id(t): t.get_end_time() for t in tracker.tracks}
            if not detections and tracker.tracks:
                stats['blank'] = True
            tracker.process(None, detections, [k.copy() for k in kps])
            for t in tracker.tracks:
                if id(t) in ends and t.get_end_time() == tracker.time - 1:
                    stats['skips'].add(int(t.get_end_time() - ends[id(t)]))
            objs = tracker.get_tracked_objects()
            rec['det_boxes'].append(boxes)
            rec['det_kps'].append(kps)
            rec['det_counts'].append(len(boxes))
            rec['out_boxes'] += [[int(v) for v in o.rect[:4]] for o in objs]
            rec['out_kps'] += [np.asarray(o.kp, dtype=np.float64).reshape(18) for o in objs]
            rec['out_ids'] += [int(o.label.split()[1]) for o in objs]
            rec['out_counts'].append(len(objs))
            rec['num_tracks'].append(len(tracker.tracks))
            rec['last_global_id'].append(tracker.last_global_id)
            stats['max_live'] = max(stats['max_live'], len(tracker.tracks))
    finally:
        mod.linear_sum_assignment, mod.IOUTracker._iou, mod.Track._filter_last_3d_box = o_lsa, o_iou, o_filter
    stats['skips'].discard(0)
    stats['cleared'], stats['last_global_id'] = len(tracker.history_tracks), tracker.last_global_id
    arrays = dict(det_boxes=np.concatenate(rec['det_boxes']).astype(np.int32).reshape(-1, 4),
                  det_kps=np.concatenate(rec['det_kps']).astype(np.float32).reshape(-1, 18),
                  det_counts=np.array(rec['det_counts'], np.int32),
                  out_boxes=np.array(rec['out_boxes'], np.int32).reshape(-1, 4),
                  out_kps=np.array(rec['out_kps'], np.float64).reshape(-1, 18), out_ids=np.array(rec['out_ids'], np.int32),
                  out_counts=np.array(rec['out_counts'], np.int32), num_tracks=np.array(rec['num_tracks'], np.int32),
                  last_global_id=np.array(rec['last_global_id'], np.int32))
    return arrays, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the reference project')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'tracker.npz'))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location(
        'reference_tracking_tools', os.path.join(args.reference, 'torchdet3d', 'utils', 'tracking_tools.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    # seeds: the first SEEDS_PER_SET whose margins hold under every parameter set
    seeds, runs, seed = [], {}, 0
    while len(seeds) < SEEDS_PER_SET:
        assert seed < 64, 'no usable seeds'
        scene = make_scene(seed, FRAMES, blank_frame=24 + seed % 5)
        res = {name: run_scene(mod, dict(DEFAULTS, **over), scene) for name, over in SETS.items()}
        worst = min(min(st['cost'], st['iou'], st['kp'], st['gap']) for _, st in res.values())
        print(f'seed {seed}: smallest margin {worst:.3g}' + ('' if worst >= MARGIN else '  (skipped)'))
        if worst >= MARGIN:
            seeds.append(seed)
            runs[seed] = res
        seed += 1

    out, names, allst = {}, [], []
    for name, over in SETS.items():
        params = dict(DEFAULTS, **over)
        for seed in seeds:
            arrays, st = runs[seed][name]
            k = len(names)
            names.append(f'{name}/seed{seed}')
            allst.append(st)
            out[f's{k}_params_int'] = np.array([params[n] for n in ('time_window', 'continue_time_thresh', 'track_clear_thresh',
                                                                    'interpolate_time_thresh', 'no_updated_frames_treshold',
                                                                    'align_kp')], np.int32)
            out[f's{k}_params_float'] = np.array([params[n] for n in ('match_threshold', 'track_detection_iou_thresh',
                                                                      'detection_filter_speed', 'keypoints_filter_speed',
                                                                      'add_treshold')], np.float64)
            for key, v in arrays.items():               # (the inputs of a seed are stored once, not once per parameter set)
                out[f'in{seed}_{key}' if key.startswith('det_') else f's{k}_{key}'] = v
            out[f's{k}_seed'] = np.array(seed, np.int32)
            print(f'{names[-1]}: margins cost {st["cost"]:.2g} iou {st["iou"]:.2g} kp {st["kp"]:.2g} assignment {st["gap"]:.2g}; '
                  f'skips {sorted(st["skips"])}, largest matrix {st["max_matrix"]}, no_updated_frames up to {st["nouf"]}, '
                  f'last_global_id {st["last_global_id"]}, live tracks <= {st["max_live"]}, cleared {st["cleared"]}, '
                  f'id reuse {st["reuse"]}')
    for key in ('cost', 'iou', 'kp', 'gap'):
        assert min(st[key] for st in allst) >= MARGIN, key
    assert any(st['reuse'] for st in allst), 'no scene reuses a released id'
    assert any(st['cleared'] for st in allst), 'no track leaves through track_clear_thresh'
    assert any(st['more'] for st in allst) and any(st['fewer'] for st in allst), 'assignment matrices rectangular one way only'
    assert any(st['blank'] for st in allst), 'no frame without detections while tracks are live'
    out['names'] = np.array(names)
    np.savez_compressed(args.out, **out)
    print(f'wrote {args.out}: {len(names)} scenes, {os.path.getsize(args.out)} bytes')


if __name__ == '__main__':
    main()
