"""Loader boundary (torchdet3d/builders/loader_builder.py:14-68 of the reference).

`cfg.data.root == 'synthetic'`: `SyntheticCrops`, batches `(imgs f32 [B,3,H,W] normalised, gt_kp f32 [B,9,2] in [0,1], gt_cats
int64 [B])` -- the reference's output contract (objectron_main.py:51-96 + utils/transforms.py:103-114) without a dataset.
Any other root: the Objectron dataset (dataloaders/objectron.py) with the config's pipelines compiled by
`build_augmentations` and applied on the GPU (`GpuAugmentLoader`, one `t3d_augment_crops_u8` launch per batch): batches
`(imgs uint8 [B,oh,ow,3] NHWC on the device, gt_kp f32 [B,9,2], gt_cats int64 [B])`, normalised inside the stem.
`cfg.data.cache = 'device'` (budget `cfg.data.cache_max_gb`, default 32): each of the three loaders decodes its dataset once,
keeps the resized crops in device memory and serves every epoch from there (`t3d_augment_resized_u8`), the same batches
bit for bit; under several ranks each rank caches the dataset it was given.

One process per GPU (an unchanged scripts/main.py under `python -m torch.distributed.run`; `build_model`, called first by
main.py:46, has joined the process group by the time main.py:63 builds the loaders): the reference's `nn.DataParallel`
scatters ONE batch of `train_batch_size` crops over the replicas (main.py:60-61), so here every rank draws its own
`train_batch_size / world` share of the same global batch -- `DistributedSampler` over the one dataset every rank holds
(same shuffle seed, disjoint index sets, `set_epoch` called by `Trainer.train`) -- and validation walks the samples
`rank, rank + world, ...` without padding (the per-rank partial sums are all-reduced by `Evaluator.val`)."""
import torch

from ..parallel import rank, world_size


class SyntheticCrops(torch.utils.data.Dataset):
    def __init__(self, n, size=(224, 224), num_classes=9, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.imgs = torch.randn(n, 3, size[1], size[0], generator=g)
        self.kp = torch.rand(n, 9, 2, generator=g)
        self.cats = torch.randint(0, max(num_classes, 1), (n,), generator=g)

    def __len__(self):
        return self.imgs.shape[0]

    def __getitem__(self, i):
        return self.imgs[i], self.kp[i], self.cats[i]


def build_loader(config, mode='train'):
    if config.data.root != 'synthetic':
        return _build_objectron_loaders(config)
    n = config.data.synthetic_len or 64
    size = tuple(config.data.resize) if config.data.resize else (224, 224)
    mk = lambda seed: SyntheticCrops(n, size, config.model.num_classes or 9, seed)
    tb, vb = config.data.train_batch_size or 8, config.data.val_batch_size or 8
    world, rk = world_size(), rank()
    if world == 1:
        train = torch.utils.data.DataLoader(mk(1), batch_size=tb, shuffle=True, drop_last=True)
        val = torch.utils.data.DataLoader(mk(2), batch_size=vb, shuffle=False)
    else:
        if tb % world:
            raise ValueError(f'data.train_batch_size = {tb} is the GLOBAL batch (scripts/main.py:60-61 scatters it over the '
                             f'replicas): it must be divisible by the {world} ranks of this launch')
        ds = mk(1)
        seed = int(getattr(getattr(config, 'utils', None), 'random_seeds', 0) or 0)
        sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=world, rank=rk, shuffle=True, seed=seed,
                                                                  drop_last=True)
        train = torch.utils.data.DataLoader(ds, batch_size=tb // world, sampler=sampler, drop_last=True)
        dv = mk(2)
        val = torch.utils.data.DataLoader(torch.utils.data.Subset(dv, range(rk, len(dv), world)),
                                          batch_size=max(vb // world, 1), shuffle=False)
    test = torch.utils.data.DataLoader(mk(3), batch_size=1, shuffle=False)
    return train, val, test


def _build_objectron_loaders(config):
    from ..dataloaders import GpuAugmentLoader, Objectron, build_augmentations
    train_tf, test_tf = build_augmentations(config)
    root, cats = config.data.root, config.data.category_list or 'all'
    tb, vb = config.data.train_batch_size or 8, config.data.val_batch_size or 8
    nw = config.data.num_workers or 0
    seed = int(getattr(getattr(config, 'utils', None), 'random_seeds', 0) or 0)
    cache = dict(cache=config.data.cache or None, cache_max_gb=config.data.cache_max_gb or 32)
    world, rk = world_size(), rank()
    if tb % world:
        raise ValueError(f'data.train_batch_size = {tb} is the GLOBAL batch (scripts/main.py:60-61 scatters it over the '
                         f'replicas): it must be divisible by the {world} ranks of this launch')
    ds = Objectron(root, mode='train', transform=train_tf, category_list=cats)
    # a shuffle that depends on (seed, epoch) only -- one rank is a DistributedSampler of one replica
    sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=world, rank=rk, shuffle=True, seed=seed,
                                                              drop_last=True)
    train = GpuAugmentLoader(ds, train_tf, tb // world, sampler=sampler, num_workers=nw, drop_last=True, seed=seed, rank=rk,
                             **cache)
    dv = Objectron(root, mode='val', transform=test_tf, category_list=cats)
    if world > 1:
        dv = torch.utils.data.Subset(dv, range(rk, len(dv), world))
    val = GpuAugmentLoader(dv, test_tf, max(vb // world, 1), num_workers=nw, seed=seed, rank=rk, **cache)
    dt = Objectron(root, mode='test', transform=test_tf, category_list=cats)
    test = GpuAugmentLoader(dt, test_tf, 1, num_workers=nw, seed=seed, rank=rk, **cache)
    return train, val, test


def _get(obj, name, default=None):
    """An entry of an mmdet-style config object: attribute (addict / Config) or key (dict)."""
    if isinstance(obj, dict):
        return obj.get(name, default)
    v = getattr(obj, name, default)
    return default if v is None else v


def build_detection_loader(cfg):
    """The detector's loaders from an mmdet-style config object (the shape of configs/detection/mnv2_ssd_300_2_heads.py:63-143;
    attributes or keys): `input_size`, `train_pipeline`, `test_pipeline`, `data.samples_per_gpu`, `data.workers_per_gpu`,
    `data.train.dataset.{ann_file, img_prefix, min_size, classes}` (a `RepeatDataset` wrapper with times=1; `data.train` itself
    may also be the dataset), `data.val.{ann_file, img_prefix}`; optional `seed`; optional `data.decode` ('host', the default: Pillow in the workers; 'device':
    the workers read file bytes and the frames are decoded on the GPU, dataloaders/jpeg.py), `data.decode_index` (a path stem:
    the JPEG indexes are kept in `<stem>.train.npy` / `<stem>.val.npy`, built when missing) and `data.decode_seg_mcus`;
    optional `data.cache` ('device': the files, their JPEG index and the annotations are kept in GPU memory and every batch is
    decoded, drawn and augmented there, dataloaders/detection_arena.py -- it implies the index, `data.decode_index` and
    `data.decode_seg_mcus` apply as for decode='device', `workers_per_gpu` is not used; any other value raises ValueError) with
    its budget `data.cache_max_gb` (GiB, default 32: a set that does not fit raises before anything is allocated); optional
    `data.decode_crop` (default off; with `data.cache = 'device'` only, ValueError without it: the train loader decodes of every
    frame only the part its drawn crop reads -- `ArenaDetectionLoader(crop_decode=True)` -- the same batches bit for bit).
    -> (train, val) `GpuDetectionLoader`s, or `ArenaDetectionLoader`s with `data.cache = 'device'` (the same tuples bit for bit,
    but G is the largest box count of the SET, not of the batch; each rank holds the whole arena):
    train yields (imgs uint8 [B,S,S,3], gt_boxes, gt_labels, gt_counts), shuffled by (seed, epoch), last partial batch dropped;
    val is the test pipeline (the resize alone) in dataset order and also yields ori_shapes.  `samples_per_gpu` is PER RANK,
    as in mmdet; under several ranks train uses a DistributedSampler over the one dataset every rank holds and val walks the
    images rank, rank + world, ... without padding, as `_build_objectron_loaders` does."""
    from ..dataloaders import DetectionAugmentPipeline, GpuDetectionLoader, ObjectronFrames
    from ..utils import OBJECTRON_CLASSES
    s = int(_get(cfg, 'input_size', 300))
    data = _get(cfg, 'data')
    bs, nw = int(_get(data, 'samples_per_gpu', 1)), int(_get(data, 'workers_per_gpu', 0))
    seed = int(_get(cfg, 'seed', 0) or 0)
    tr = _get(data, 'train')
    if _get(tr, 'dataset') is not None:
        if int(_get(tr, 'times', 1)) != 1:
            raise NotImplementedError(f'data.train.times = {_get(tr, "times")} is not built (RepeatDataset with times=1 only)')
        tr = _get(tr, 'dataset')
    classes = _get(tr, 'classes')
    cats = 'all' if classes is None or list(classes) == list(OBJECTRON_CLASSES) else list(classes)
    train_tf = DetectionAugmentPipeline(_get(cfg, 'train_pipeline'), (s, s))
    test_tf = DetectionAugmentPipeline(_get(cfg, 'test_pipeline'), (s, s))
    if test_tf.random:
        raise NotImplementedError('test_pipeline: only the Resize alone is built')
    world, rk = world_size(), rank()
    decode = _get(data, 'decode', 'host')
    cache = _get(data, 'cache')
    if cache is not None and cache != 'device':
        raise ValueError(f"data.cache = {cache!r}: only 'device' (files, index and annotations kept in GPU memory) or nothing is built")
    if cache:
        decode = 'device'
    decode_crop = bool(_get(data, 'decode_crop', False))
    if decode_crop and not cache:
        raise ValueError("data.decode_crop = True needs data.cache = 'device': only the arena loader, which draws the crops on the "
                         'device before it decodes, can decode the drawn crop alone')
    stem, seg_mcus = _get(data, 'decode_index'), _get(data, 'decode_seg_mcus')

    def indexed(d, which):
        if decode == 'device':
            d.build_index(None if stem is None else f'{stem}.{which}.npy', threads=16, seg_mcus=seg_mcus)
        return d
    ds = indexed(ObjectronFrames(_get(tr, 'img_prefix'), 'train', cats, int(_get(tr, 'min_size', 17) or 0),
                                 ann_file=_get(tr, 'ann_file'), decode=decode), 'train')
    sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=world, rank=rk, shuffle=True, seed=seed,
                                                              drop_last=True)
    va = _get(data, 'val')
    dv = indexed(ObjectronFrames(_get(va, 'img_prefix'), 'val', cats, ann_file=_get(va, 'ann_file'), decode=decode), 'val')
    if cache:
        from ..dataloaders.detection_arena import ArenaDetectionLoader, DetectionArena
        max_gb = _get(data, 'cache_max_gb', 32) or 32
        arenas = [DetectionArena(d, max_gb) for d in (ds, dv)]          # (both planned -- budget, box capacity -- before either is filled)
        for a in arenas:
            a.fill()
        train = ArenaDetectionLoader(arenas[0], train_tf, bs, sampler=sampler, drop_last=True, seed=seed, rank=rk,
                                     crop_decode=decode_crop)
        sub = torch.utils.data.Subset(dv, range(rk, len(dv), world)) if world > 1 else dv
        val = ArenaDetectionLoader(arenas[1], test_tf, bs, indices=range(rk, len(dv), world), seed=seed, rank=rk, dataset=sub)
        return train, val
    train = GpuDetectionLoader(ds, train_tf, bs, sampler=sampler, num_workers=nw, drop_last=True, seed=seed, rank=rk)
    if world > 1:
        dv = torch.utils.data.Subset(dv, range(rk, len(dv), world))
    val = GpuDetectionLoader(dv, test_tf, bs, num_workers=nw, seed=seed, rank=rk)
    return train, val
