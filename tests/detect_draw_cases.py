"""The cases `t3d_detect_draw_host` is held to numpy over (tests/test_detect_draw_host.py) and `t3d_detect_draw` to
`t3d_detect_draw_host` (tests/test_gpu_detect_draw.py): the smallest that still reach every branch -- frames of 33 x 17 and
100 x 130 and one of 1440 x 1920; one mid box, one large box, two tiny far-apart boxes (the search then restarts its mode
loop), an image at the table's capacity of 64 boxes; keys with batch 0 and a batch above 65 535, rank 1 and a seed above 2^32; the config's training
pipeline, one without Expand, one without the crop, one with Resize and flip only -- and the host reference: the pipeline's own
draw / boxes / records with a counting wrapper around the crop search's generator."""
import numpy as np

CONFIG = [
    dict(type='LoadImageFromFile', to_float32=True),
    dict(type='LoadAnnotations', with_bbox=True),
    dict(type='PhotoMetricDistortion', brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18),
    dict(type='Albu', transforms=[dict(type='RandomRotate90and270', p=0.5)], update_pad_shape=False, skip_img_without_anno=True),
    dict(type='Expand', ratio_range=(1, 3)),
    dict(type='MinIoURandomCrop', min_ious=(0.1, 0.3, 0.5, 0.7, 0.9), min_crop_size=0.1),
    dict(type='Resize', img_scale=(300, 300), keep_ratio=False),
    dict(type='Normalize', mean=[0, 0, 0], std=[255, 255, 255], to_rgb=True),
    dict(type='RandomFlip', flip_ratio=0.5),
    dict(type='DefaultFormatBundle'),
    dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels']),
]
PIPELINES = {
    'config': CONFIG,
    'no_expand': [s for s in CONFIG if s['type'] != 'Expand'],
    'no_crop': [s for s in CONFIG if s['type'] != 'MinIoURandomCrop'],
    'resize_flip': [s for s in CONFIG if s['type'] in ('LoadImageFromFile', 'LoadAnnotations', 'Resize', 'RandomFlip', 'Collect')],
}
KEYS = [(7, 0, 0, 0), (7, 3, 1, 70000), (2 ** 32 + 12345, 1, 0, 5)]
TINY = 'config/100x130/tiny2'           # the case whose search restarts its mode loop


def _boxes(kind, h, w):
    """-> per image of the case's table, float32 [n, 4]."""
    mid = np.array([[.3 * w, .3 * h, .6 * w, .65 * h]], np.float32)
    if kind == 'mid':
        return [mid]
    if kind == 'large':                     # (a crop can reach an IoU of 0.9 with it: the last mode returns too)
        return [np.array([[.05 * w, .05 * h, .95 * w, .95 * h]], np.float32)]
    if kind == 'tiny2':
        return [np.array([[3, 3, 6, 7], [120, 90, 126, 97]], np.float32)]
    rng = np.random.default_rng(11)         # 'cap': an image at capacity, between one with a single box and one with three
    x, y = rng.uniform(0, w * .7, 64), rng.uniform(0, h * .7, 64)
    full = np.stack([x, y, x + rng.uniform(1, w * .3, 64), y + rng.uniform(1, h * .3, 64)], 1).astype(np.float32)
    return [mid, full, full[:3].copy()]


def cases():
    """[dict(name, steps, key, h, w, boxes [per image float32 [n, 4]], labels [per image int32 [n]], G)]."""
    out = []
    for pipe, h, w, kind, key in (('config', 33, 17, 'mid', 0), ('config', 100, 130, 'mid', 1), ('config', 100, 130, 'tiny2', 0),
                                  ('config', 100, 130, 'cap', 2), ('config', 1440, 1920, 'mid', 1), ('config', 33, 17, 'cap', 2),
                                  ('no_expand', 100, 130, 'mid', 2), ('no_expand', 100, 130, 'tiny2', 1), ('no_crop', 33, 17, 'mid', 1),
                                  ('no_crop', 100, 130, 'cap', 0), ('resize_flip', 100, 130, 'mid', 2), ('resize_flip', 33, 17, 'cap', 1),
                                  ('no_expand', 100, 130, 'large', 0)):
        boxes = _boxes(kind, h, w)
        labels = [(np.arange(len(b), dtype=np.int32) * 5 + j) % 9 for j, b in enumerate(boxes)]
        out.append(dict(name=f'{pipe}/{h}x{w}/{kind}', steps=PIPELINES[pipe], key=KEYS[key], h=h, w=w, boxes=boxes, labels=labels,
                        G=max(len(b) for b in boxes)))
    return out


def tables(case, B):
    """-> (frames int64 [B, 4] = (offset, h, w, dataset index), boxes float32 [n, 4], labels int32 [n], box_start int64 [images + 1]):
    sample i is image i % images."""
    n = len(case['boxes'])
    idx = np.arange(B, dtype=np.int64) % n
    nb = case['h'] * case['w'] * 3
    frames = np.stack([np.arange(B, dtype=np.int64) * nb, np.full(B, case['h'], np.int64), np.full(B, case['w'], np.int64), idx], 1)
    counts = [len(b) for b in case['boxes']]
    return frames, np.concatenate(case['boxes']), np.concatenate(case['labels']), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def pipeline(case):
    from torchdet3d.dataloaders import DetectionAugmentPipeline
    return DetectionAugmentPipeline(case['steps'], (300, 300))


class _Counting:
    def __init__(self, rng):
        self.rng, self.n = rng, 0

    def random(self):
        self.n += 1
        return self.rng.random()


def host_reference(case, B):
    """The numpy pipeline over the case's B samples -> (records [B], boxes per sample, labels per sample, mode float64 [B],
    uniforms the crop search drew, int [B])."""
    pipe = pipeline(case)
    frames, _, _, _ = tables(case, B)
    drawn, search = [], pipe._min_iou_crop

    def counted(b, h, w, rng):
        c = _Counting(rng)
        out = search(b, h, w, c)
        drawn.append(c.n)
        return out
    pipe._min_iou_crop = counted
    prm = pipe.draw(B, case['key'])
    desc = frames[:, :3]
    bl, ll = pipe.boxes([case['boxes'][j] for j in frames[:, 3]], [case['labels'][j] for j in frames[:, 3]], desc, prm)
    rec = pipe.records(desc, prm)
    return rec, bl, ll, prm['mode'], np.asarray(drawn if pipe.crop is not None else [0] * B, np.int64)
