"""GPU: the device crop cache.  `t3d_augment_resized_u8` over an arena of resized crops against `t3d_augment_crops_u8` on
the crops themselves and against the numpy restatement (tests/augment_ref.py), bad records, arena offsets beyond 2^32; the
cached loader (`cfg.data.cache = 'device'`) against the uncached one batch by batch over three epochs, with and without
prefetch and workers and under a busy stream; no decode after the prefill; two ranks' shards; and scripts/main.py's flow
(Trainer.train x 2 -> Evaluator.val -> visual_test) with and without the cache.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu

SIZE = (96, 96)


@pytest.fixture(scope='module')
def root(tmp_path_factory):
    return R.write_dataset(str(tmp_path_factory.mktemp('objectron')), seed=4, n_train=16, n_test=8)


def _cfg(root, **data):
    from test_host_logic import _cfg as base
    cfg = base('mobilenetv3_large')
    cfg.model.storage_dtype = 'bf16'
    tr, te = R.default_pipelines(SIZE)
    d = dict(root=root, resize=SIZE, train_batch_size=8, val_batch_size=4, num_workers=0, category_list='all',
             normalization=R.NORMALIZATION, max_epochs=2)
    d.update(data)
    cfg.data = type(cfg)(d)
    cfg.utils = type(cfg)(dict(random_seeds=5, debug_mode=False, save_freq=10, print_freq=20, debug_steps=100))
    cfg.train_data_pipeline, cfg.test_data_pipeline = tr, te
    return cfg


def _batches(loader, epoch=0):
    if hasattr(loader.sampler, 'set_epoch'):
        loader.sampler.set_epoch(epoch)
    return [tuple(t.clone() for t in b) for b in loader]


def _same(got, ref):
    assert len(got) == len(ref) and len(ref) > 0
    for x, y in zip(got, ref):
        assert len(x) == len(y) == 3
        assert all(u.dtype == v.dtype and torch.equal(u, v) for u, v in zip(x, y))


# ---- 1. kernel against kernel ----------------------------------------------------------------------------------------------
def _call(name, src, nbytes, rec, B, oh, ow):
    from torchdet3d import _native as N
    recd = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    out = torch.full((B, oh, ow, 3), 77, dtype=torch.uint8, device='cuda')
    N.call(name, N.ptr(src), nbytes, N.ptr(recd), N.ptr(out), B, oh, ow, N.stream())
    return out


def _case(oh, ow, seed, nslot=10, B=37):
    """nslot random crops, their arena (the crops kernel with no flag set), and B records that walk the slots out of order
    and repeatedly through every flag combination: -> (crops, src, arena, rec for the crops, rec for the arena, params)."""
    from torchdet3d.dataloaders.objectron import AUG_SAMPLE_DTYPE
    rng = np.random.default_rng(seed)
    crops = [rng.integers(0, 256, (int(h), int(w), 3), dtype=np.uint8) for h, w in rng.integers(20, 301, (nslot, 2))]
    offs = np.concatenate([[0], np.cumsum([c.size for c in crops])]).astype(np.int64)
    src = torch.from_numpy(np.concatenate([c.reshape(-1) for c in crops])).cuda()
    plain = np.zeros(nslot, AUG_SAMPLE_DTYPE)
    plain['offset'], plain['h'], plain['w'] = offs[:-1], [c.shape[0] for c in crops], [c.shape[1] for c in crops]
    arena = _call('t3d_augment_crops_u8', src, src.numel(), plain, nslot, oh, ow).reshape(-1)
    slots = np.concatenate([rng.permutation(nslot), rng.integers(0, nslot, B - nslot)])
    rc, ra, prm = np.zeros(B, AUG_SAMPLE_DTYPE), np.zeros(B, AUG_SAMPLE_DTYPE), []
    for j, k in enumerate(slots):
        fl = j % 16
        p = dict(slot=int(k), flip=bool(fl & 1), swap=bool(fl & 8), alpha=1.0, beta=0.0, angle=None)
        for r, (o, h, w) in ((rc, (offs[k], crops[k].shape[0], crops[k].shape[1])), (ra, (k * oh * ow * 3, oh, ow))):
            r['offset'][j], r['h'][j], r['w'][j], r['flags'][j] = o, h, w, fl
        if fl & 2:
            p['alpha'], p['beta'] = float(rng.uniform(0.8, 1.2)), float(rng.uniform(-0.2, 0.2))
            for r in (rc, ra):
                r['alpha'][j], r['beta255'][j] = np.float32(p['alpha']), np.float32(p['beta'] * 255)
        if fl & 4:
            p['angle'] = float(rng.uniform(-10, 10))
            for r in (rc, ra):
                r['m'][j] = R.invert_affine(R.rotation_matrix(p['angle'], oh, ow)).reshape(-1)
        prm.append(p)
    return crops, src, arena, rc, ra, prm


@pytest.mark.parametrize('oh,ow', [(96, 96), (224, 224), (13, 17), (100, 75)])
def test_resized_kernel_equals_the_crops_kernel_and_the_restatement(oh, ow):
    crops, src, arena, rc, ra, prm = _case(oh, ow, seed=oh * 1000 + ow)
    B = len(rc)
    a = _call('t3d_augment_crops_u8', src, src.numel(), rc, B, oh, ow)
    b = _call('t3d_augment_resized_u8', arena, arena.numel(), ra, B, oh, ow)
    assert torch.equal(a, b), [j for j in range(B) if not torch.equal(a[j], b[j])]
    got = b.cpu().numpy()
    for j, p in enumerate(prm):
        if (oh, ow) == (224, 224) and j >= 16:
            break                                            # (the restatement is slow at this size: one of each combination)
        ref = R.augment(crops[p['slot']], oh, ow, p['flip'], p['alpha'], p['beta'], p['angle'], p['swap'])
        assert np.array_equal(got[j], ref), (j, p)


@pytest.mark.parametrize('oh,ow', [(96, 96), (13, 17)])
def test_bad_records_give_zeros_and_leave_their_neighbours(oh, ow):
    from torchdet3d import _native as N
    _, _, arena, _, ra, _ = _case(oh, ow, seed=7)
    B, slot = len(ra), oh * ow * 3
    good = _call('t3d_augment_resized_u8', arena, arena.numel(), ra, B, oh, ow)
    bad = ra.copy()
    bad['offset'][3] = -slot
    bad['offset'][4] = -1
    bad['offset'][9] = arena.numel() - slot + 1              # its last byte is one past the arena
    bad['offset'][10] = arena.numel()
    bad['h'][20] = oh + 1
    bad['w'][21] = ow - 1
    bad['h'][22], bad['w'][22] = ow, oh                      # (transposed: a zero image unless the output is square)
    zero = [3, 4, 9, 10, 20, 21] + ([22] if oh != ow else [])
    out = _call('t3d_augment_resized_u8', arena, arena.numel(), bad, B, oh, ow)
    for j in range(B):
        assert (out[j] == 0).all() if j in zero else torch.equal(out[j], good[j]), j
    # arena_bytes is the bound, not the allocation: the last slot is outside an arena declared one byte shorter
    short = _call('t3d_augment_resized_u8', arena, arena.numel() - 1, ra, B, oh, ow)
    last = arena.numel() // slot - 1
    for j in range(B):
        assert (short[j] == 0).all() if ra['offset'][j] == last * slot else torch.equal(short[j], good[j]), j
    with pytest.raises(RuntimeError):
        N.call('t3d_augment_resized_u8', N.ptr(arena), arena.numel(), N.ptr(good), N.ptr(out), B, 0, ow, N.stream())
    with pytest.raises(RuntimeError):
        N.call('t3d_augment_resized_u8', N.ptr(arena), 0, N.ptr(good), N.ptr(out), B, oh, ow, N.stream())


# ---- 2. offsets beyond 2^32 ------------------------------------------------------------------------------------------------
def test_arena_offsets_beyond_32_bits():
    from torchdet3d.dataloaders.objectron import AUG_SAMPLE_DTYPE
    free = torch.cuda.mem_get_info()[0]
    if free < 8e9:
        pytest.skip(f'{free / 1e9:.1f} GB of device memory free: the 4.3 GB arena of this test wants 8 GB')
    oh = ow = 224
    slot = oh * ow * 3
    nslot = int(4.3e9) // slot + 8
    assert (nslot - 3) * slot > 2 ** 32
    rng = np.random.default_rng(1)
    imgs = torch.from_numpy(rng.integers(0, 256, (3, oh, ow, 3), dtype=np.uint8)).cuda()
    big = torch.empty(nslot * slot, dtype=torch.uint8, device='cuda')
    big[(nslot - 3) * slot:].copy_(imgs.reshape(-1))
    big[:3 * slot].fill_(9)                                  # what a truncated offset would read
    B = 16
    rs, rb = np.zeros(B, AUG_SAMPLE_DTYPE), np.zeros(B, AUG_SAMPLE_DTYPE)
    for j in range(B):
        for r, base in ((rs, 0), (rb, nslot - 3)):
            r['offset'][j], r['h'][j], r['w'][j], r['flags'][j] = (base + j % 3) * slot, oh, ow, j
            r['alpha'][j], r['beta255'][j] = 1.1, -9.0
            r['m'][j] = R.invert_affine(R.rotation_matrix(3.0 + j, oh, ow)).reshape(-1)
    small = imgs.reshape(-1)
    a = _call('t3d_augment_resized_u8', small, small.numel(), rs, B, oh, ow)
    b = _call('t3d_augment_resized_u8', big, big.numel(), rb, B, oh, ow)
    assert torch.equal(a, b) and torch.equal(b[0], imgs[0]) and not (b == 0).all(dim=3).all()
    del big
    torch.cuda.empty_cache()


# ---- 3. loader equality ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prefetch,workers', [(0, 0), (0, 2), (2, 0), (2, 2)])
def test_cached_loader_equals_uncached(root, prefetch, workers):
    from torchdet3d.builders import build_loader
    plain = build_loader(_cfg(root, num_workers=workers))
    cached = build_loader(_cfg(root, num_workers=workers, cache='device'))
    for ld in plain + cached:
        ld.prefetch = prefetch
    for which in (0, 1):                                     # train (random pipeline, shuffled, drop_last) and val
        assert cached[which]._arena is None
        for epoch in (0, 1, 2):
            _same(_batches(cached[which], epoch), _batches(plain[which], epoch))
        n = len(cached[which].dataset)
        assert cached[which]._arena.numel() == n * SIZE[0] * SIZE[1] * 3 and cached[which]._c_kp.shape == (n, 9, 2)
    assert plain[0].pipeline.is_random
    assert not torch.equal(_batches(cached[0], 0)[0][0], _batches(cached[0], 1)[0][0])      # another epoch: another draw


def test_cached_prefetch_under_a_busy_stream_and_odd_slot_size(root):
    from torchdet3d.builders import build_loader
    sync = build_loader(_cfg(root))[0]
    sync.prefetch = 0
    ref = _batches(sync, 1)
    c = build_loader(_cfg(root, num_workers=2, cache='device'))[0]
    c.prefetch = 2
    c.fill_cache()                                           # the public prefill
    arena = c._arena
    c.sampler.set_epoch(1)
    torch.cuda.synchronize()
    torch.cuda._sleep(100_000_000)                 # the consumer's stream runs ~50 ms behind while the loader enqueues
    got = [b for b in c]
    torch.cuda.synchronize()
    _same(got, ref)
    assert c._arena is arena                                 # filled once
    # a slot size that is not a multiple of 4 (13 x 17 x 3 = 663): the prefill stages what the kernel cannot store in place
    tr, te = R.default_pipelines((13, 17))
    for cache in (None, 'device'):
        cfg = _cfg(root, resize=(13, 17), train_batch_size=5, cache=cache)
        cfg.train_data_pipeline, cfg.test_data_pipeline = tr, te
        ld = build_loader(cfg)[0]
        out = [_batches(ld, e) for e in (0, 1)]
        if cache is None:
            want = out
    for g, w in zip(out, want):
        _same(g, w)


# ---- 4. no decode after the prefill ----------------------------------------------------------------------------------------
def test_frames_are_decoded_once(root, monkeypatch):
    from torchdet3d.builders import build_loader
    from torchdet3d.dataloaders import Objectron
    calls = []
    load = Objectron.load_image

    def counted(self, indx):
        calls.append(indx)
        return load(self, indx)

    monkeypatch.setattr(Objectron, 'load_image', counted)
    train = build_loader(_cfg(root, num_workers=0, cache='device'))[0]
    n = len(train.dataset)
    assert len(_batches(train, 0)) == n // 8 and len(calls) == n and sorted(calls) == list(range(n))
    for epoch in (1, 2):
        _batches(train, epoch)
    assert len(calls) == n
    plain = build_loader(_cfg(root, num_workers=0))[0]
    _batches(plain, 0)
    assert len(calls) == n + n // 8 * 8                      # (the uncached loader decodes every object it serves)


# ---- 5. two ranks without a process group ----------------------------------------------------------------------------------
def test_two_ranks_shards_cached_equals_uncached(root):
    from torch.utils.data.distributed import DistributedSampler
    from torchdet3d.dataloaders import GpuAugmentLoader, Objectron, build_augmentations
    pipe = build_augmentations(_cfg(root))[0]
    seen = []
    for r in (0, 1):
        pair = []
        for cache in (None, 'device'):
            ds = Objectron(root, mode='train', transform=pipe)
            sampler = DistributedSampler(ds, num_replicas=2, rank=r, shuffle=True, seed=5, drop_last=True)
            pair.append(GpuAugmentLoader(ds, pipe, 4, sampler=sampler, drop_last=True, seed=5, rank=r, cache=cache))
        for epoch in (0, 1):
            ref = _batches(pair[0], epoch)
            _same(_batches(pair[1], epoch), ref)
            if epoch == 0:
                seen.append(ref)
    assert not torch.equal(seen[0][0][0], seen[1][0][0])     # the ranks serve different shards with different draws


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------
def _main_flow(root, tmp_path, cache):
    from test_boundary_main import _Writer
    from torchdet3d.builders import build_loader, build_loss, build_model, build_optimizer, build_scheduler
    from torchdet3d.evaluation import Evaluator
    from torchdet3d.losses import LossManager
    from torchdet3d.trainer import Trainer
    from torchdet3d.utils import set_random_seed
    cfg = _cfg(root, cache=cache)
    set_random_seed(cfg.utils.random_seeds)
    net = build_model(cfg).to('cuda')
    opt = build_optimizer(cfg, net)
    sched = build_scheduler(cfg, opt)
    lm = LossManager(build_loss(cfg), cfg.loss.coeffs, cfg.loss.alwa)
    train_loader, val_loader, test_loader = build_loader(cfg)
    assert train_loader.cache == cache
    writer = _Writer()
    tr = Trainer(model=net, train_loader=train_loader, optimizer=opt, scheduler=sched, loss_manager=lm, writer=writer,
                 max_epoch=2, log_path=str(tmp_path), device='cuda', save_chkpt=False, print_freq=1)
    ev = Evaluator(model=net, val_loader=val_loader, test_loader=test_loader, cfg=cfg, writer=writer, device='cuda',
                   max_epoch=2, path_to_save_imgs=str(tmp_path), samples=[0, 3, 5], num_samples=3)
    res = [{k: v for k, v in dict(tr.train(epoch, epoch == 1)).items() if k != 'time'} for epoch in range(2)]   # (wall clock)
    assert tr._sp is not None and tr._sp.replays > 0
    st = opt.state[net.flat]
    state = (net.flat.detach().clone(), st['exp_avg'].clone(), st['exp_avg_sq'].clone())
    val = dict(ev.val(1))
    vis = ev.visual_test()
    assert len(vis) == 3 and all(np.isfinite(r['ADD']) for r in vis)
    item = test_loader.dataset[0]
    assert len(item) == 5 and item[0].ndim == 3 and item[1].is_cuda and tuple(item[1].shape) == SIZE + (3,)
    return res, state, val, vis, [s for s in writer.scalars]


def test_training_and_validation_identical_with_and_without_the_cache(root, tmp_path):
    ra, sa, va, visa, wa = _main_flow(root, tmp_path, None)
    rb, sb, vb, visb, wb = _main_flow(root, tmp_path, 'device')
    assert all(np.isfinite(v) for r in ra for v in r.values()) and all('loss' in r for r in ra)
    assert ra == rb, (ra, rb)
    for x, y in zip(sa, sb):
        assert torch.equal(x, y)
    assert va == vb and all(np.isfinite(v) for v in va.values())
    assert [(r['idx'], r['ADD'], r['SADD'], r['accuracy']) for r in visa] == [(r['idx'], r['ADD'], r['SADD'], r['accuracy'])
                                                                             for r in visb]
    assert len(wa) == len(wb) and all(a[1] == b[1] or (a[1] != a[1] and b[1] != b[1]) for a, b in zip(wa, wb))
