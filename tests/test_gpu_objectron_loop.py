"""GPU: the Objectron loader in the training loop.  scripts/main.py's flow on a tiny dataset with the reference's default
pipelines (build_loader -> Trainer.train x 2 -> Evaluator.val -> visual_test), reproducible uint8 NHWC device batches, the
prefetched loader equal to a synchronous one under a busy stream, and a train step on a loader batch equal, bit for bit, to
one on the same crops built by the numpy restatement (tests/augment_ref.py) and uploaded."""
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
    tr, te = R.default_pipelines(SIZE)
    d = dict(root=root, resize=SIZE, train_batch_size=8, val_batch_size=4, num_workers=0, category_list='all',
             normalization=R.NORMALIZATION, max_epochs=2)
    d.update(data)
    cfg.data = type(cfg)(d)
    cfg.utils = type(cfg)(dict(random_seeds=5, debug_mode=False, save_freq=10, print_freq=20, debug_steps=100))
    cfg.train_data_pipeline, cfg.test_data_pipeline = tr, te
    return cfg


def _batches(loader, epoch=0):
    loader.sampler.set_epoch(epoch)
    return [tuple(t.clone() for t in b) for b in loader]


def test_main_flow_on_objectron(root, tmp_path):
    from test_boundary_main import _Writer
    from torchdet3d.builders import build_loader, build_loss, build_model, build_optimizer, build_scheduler
    from torchdet3d.evaluation import Evaluator
    from torchdet3d.losses import LossManager
    from torchdet3d.trainer import Trainer
    from torchdet3d.utils import set_random_seed
    cfg = _cfg(root)
    set_random_seed(cfg.utils.random_seeds)
    net = build_model(cfg).to('cuda')
    opt = build_optimizer(cfg, net)
    sched = build_scheduler(cfg, opt)
    lm = LossManager(build_loss(cfg), cfg.loss.coeffs, cfg.loss.alwa)
    train_loader, val_loader, test_loader = build_loader(cfg)
    writer = _Writer()
    tr = Trainer(model=net, train_loader=train_loader, optimizer=opt, scheduler=sched, loss_manager=lm, writer=writer,
                 max_epoch=2, log_path=str(tmp_path), device='cuda', save_chkpt=False, print_freq=1)
    ev = Evaluator(model=net, val_loader=val_loader, test_loader=test_loader, cfg=cfg, writer=writer, device='cuda',
                   max_epoch=2, path_to_save_imgs=str(tmp_path), num_samples=3)
    assert len(train_loader) == len(train_loader.dataset) // 8 == 3
    for epoch in range(2):
        res = tr.train(epoch, epoch == 1)
        assert all(np.isfinite(v) for v in res.values())
    assert tr._sp is not None and tr._sp.replays > 0                  # the step plan took the loader's batches
    val = ev.val(1)
    assert all(np.isfinite(v) for v in val.values())
    vis = ev.visual_test()
    assert len(vis) == 3 and all(np.isfinite(r['ADD']) for r in vis)
    assert all(v == v for _, v, _ in writer.scalars)
    item = test_loader.dataset[0]
    assert len(item) == 5 and item[1].is_cuda and item[1].dtype == torch.uint8 and tuple(item[1].shape) == SIZE + (3,)


def test_step_plan_is_taken_on_loader_batches(root):
    from test_gpu_step_plan import _objects
    from torchdet3d.builders import build_loader
    model, opt, lm, tr = _objects('mobilenetv3_large', 'bf16')
    train, _, _ = build_loader(_cfg(root))
    for epoch in range(3):
        train.sampler.set_epoch(epoch)
        for i, (imgs, kp, cats) in enumerate(train):
            assert imgs.is_cuda and imgs.dtype == torch.uint8 and imgs.shape == (8,) + SIZE + (3,)
            assert kp.dtype == torch.float32 and kp.shape == (8, 9, 2) and cats.dtype == torch.int64
            assert tr._step_plan().accepts(imgs, kp, cats)
            r = tr.train_step(imgs, kp, cats, i)
            assert np.isfinite(r['loss'])
    assert tr._sp.replays > 0


def test_batches_reproducible_and_prefetch_equals_synchronous(root):
    from torchdet3d.builders import build_loader
    a = build_loader(_cfg(root))[0]
    b = build_loader(_cfg(root))[0]
    for epoch in (0, 1):
        ba, bb = _batches(a, epoch), _batches(b, epoch)
        assert len(ba) == 3
        for x, y in zip(ba, bb):
            assert all(torch.equal(u, v) for u, v in zip(x, y))
    assert not torch.equal(_batches(a, 0)[0][0], _batches(a, 1)[0][0])            # another epoch: another shuffle / draw
    sync = build_loader(_cfg(root))[0]
    sync.prefetch = 0
    ref = _batches(sync, 1)
    c = build_loader(_cfg(root, num_workers=2))[0]
    c.prefetch = 2
    c.sampler.set_epoch(1)
    torch.cuda.synchronize()
    torch.cuda._sleep(100_000_000)                 # the consumer's stream runs ~50 ms behind while the loader enqueues
    got = [b for b in c]
    torch.cuda.synchronize()
    for x, y in zip(got, ref):
        assert all(torch.equal(u, v) for u, v in zip(x, y))


def test_train_step_on_a_loader_batch_equals_the_restatement(root):
    from test_gpu_step_plan import _objects
    from torchdet3d.builders import build_loader
    loader = build_loader(_cfg(root))[0]
    loader.sampler.set_epoch(1)
    imgs, kp, cats = next(iter(loader))
    # the same host batch and the same draws, finished by the numpy restatement
    loader.sampler.set_epoch(1)
    packed, desc, kp64, hcats = next(iter(loader.loader))
    prm = loader.pipeline.draw(len(desc), (5, 1, 0, 0))
    assert prm['flip'].any() or prm['rot'].any() or prm['lut'].any()
    ref_imgs, ref_kp = [], []
    for i, (o, h, w) in enumerate(desc.tolist()):
        crop = packed[o:o + h * w * 3].numpy().reshape(h, w, 3)
        ang = float(prm['angle'][i]) if prm['rot'][i] else None
        lut = bool(prm['lut'][i])
        ref_imgs.append(R.augment(crop, *SIZE, bool(prm['flip'][i]), float(prm['alpha'][i]) if lut else 1.0,
                                  float(prm['beta'][i]) if lut else 0.0, ang))
        ref_kp.append(R.keypoints(kp64[i].numpy(), h, w, *SIZE, bool(prm['flip'][i]), ang))
    ref_imgs = torch.from_numpy(np.stack(ref_imgs)).cuda()
    ref_kp, ref_cats = torch.from_numpy(np.stack(ref_kp)).cuda(), hcats.cuda()
    assert torch.equal(imgs, ref_imgs) and torch.equal(kp, ref_kp) and torch.equal(cats, ref_cats)
    outs = []
    for x, k, c in ((imgs, kp, cats), (ref_imgs, ref_kp, ref_cats)):
        model, opt, lm, tr = _objects('mobilenetv3_large', 'bf16')
        r = dict(tr.train_step(x, k, c, 0))
        st = opt.state[model.flat]
        outs.append((r['loss'], model.flat.detach().clone(), st['exp_avg'].clone(), st['exp_avg_sq'].clone()))
    (la, wa, ma, va), (lb, wb, mb, vb) = outs
    assert la == lb and np.isfinite(la)
    assert torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(wa, wb)     # gradient moments: the gradient itself
