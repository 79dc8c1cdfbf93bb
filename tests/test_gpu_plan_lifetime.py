"""Lifetime of what a recorded plan points at (torchdet3d/trainer/step_plan.py: StepPlan, ForwardPlan).

A plan stores every non-slot pointer argument as a plain 64-bit word.  The memory behind such a word has to stay allocated
for as long as the plan can be replayed: a word left pointing at a freed block makes the replay read (or, for the
descriptor of `t3d_zero_batched`, write through) whatever the caching allocator put there next.  The reference's loop
(scripts/main.py) validates at a batch size other than the training one, with a partial last batch, between two training
epochs: that is the schedule below, with the plans' pointers checked against the allocator after every phase -- before
the next replay, so a dangling word is reported without ever being replayed."""
import ctypes

import pytest
import torch

from test_gpu_step_plan import _batches
from test_host_logic import _cfg


# ---- which words a plan holds, and whether the memory behind them is still allocated ---------------------------------------
def _block_at(segments, addr):
    """The allocator's view of `addr` in a `torch.cuda.memory_snapshot()`: None outside every segment, else the state of the
    block that contains it ('active_allocated', 'inactive', ...)."""
    for s in segments:
        base = s['address']
        if not base <= addr < base + s['total_size']:
            continue
        off = base
        for b in s['blocks']:
            start = b.get('address', off)
            if start <= addr < start + b['size']:
                return b['state']
            off = start + b['size']
        return 'unmapped'
    return None


class PlanPointers:
    """Wraps `PlanRecorder.add_call` (the original still runs) and keeps (recorder, op name, argument index, address) for every
    non-null pointer argument that is recorded as a plain word: not bound to a slot, not a structure (kinds == 1).

    `check(recorders)` holds the words of the given plans against the caching allocator: an address inside one of its segments
    must lie in a block that is allocated now AND has not been freed since the plan was recorded (a freed block the allocator
    has handed to another tensor reads as allocated again).  Addresses outside every segment (library-owned memory, pinned
    host memory) are counted, not judged."""

    def __init__(self, monkeypatch):
        from torchdet3d import _native as N
        self.rows, self.mark = [], {}
        orig_add, orig_end = N.PlanRecorder.add_call, N.PlanRecorder.end_segment
        rows, mark = self.rows, self.mark

        def add_call(rec, name, args, nbytes, slots):
            orig_add(rec, name, args, nbytes, slots)
            for i, (t, v) in enumerate(zip(N.SIGNATURES[name], args)):
                if t is not N._P or v is None or isinstance(v, ctypes.Structure) or (slots and i in slots):
                    continue
                a = int(v)
                if a and a not in rec.ptr_slots:
                    rows.append((rec, name, i, a))

        def end_segment(rec):
            mark.setdefault(id(rec), len(_traces()))     # (frees from here on happened while the plan holds the word)
            return orig_end(rec)

        monkeypatch.setattr(N.PlanRecorder, 'add_call', add_call)
        monkeypatch.setattr(N.PlanRecorder, 'end_segment', end_segment)
        torch.cuda.memory._record_memory_history(enabled='all', context=None, stacks='python', max_entries=1 << 22)

    def stop(self):
        torch.cuda.memory._record_memory_history(enabled=None)

    def check(self, recorders, where):
        recs = [r for r in recorders if r is not None and r.plan]
        ids = {id(r) for r in recs}
        snap = torch.cuda.memory._snapshot()
        segs, traces = snap['segments'], _traces(snap)
        bad, outside, n = [], 0, 0
        for rec, name, i, a in self.rows:
            if id(rec) not in ids:
                continue
            n += 1
            state = _block_at(segs, a)
            if state is None:
                outside += 1
                continue
            freed = _freed_after(traces, self.mark.get(id(rec), 0), a)
            if state != 'active_allocated' or freed:
                bad.append((hex(rec.plan.value or 0), name, i, hex(a), state + (' (freed since recorded)' if freed else '')))
        print(f'[plan liveness {where}] {len(recs)} plan(s), {n} pointer words, {outside} outside the caching allocator')
        assert n > 0 or not recs
        assert not bad, f'{where}: recorded plans point at freed memory: {bad[:8]}'


def _traces(snap=None):
    snap = snap if snap is not None else torch.cuda.memory._snapshot()
    dev = torch.cuda.current_device()
    tr = snap.get('device_traces', [])
    return tr[dev] if dev < len(tr) else []


def _freed_after(traces, start, addr):
    for e in traces[start:]:
        if e['action'] in ('free_requested', 'free_completed') and e['addr'] <= addr < e['addr'] + e['size']:
            return True
    return False


def test_block_lookup_on_a_hand_made_snapshot():
    segs = [{'address': 0x1000, 'total_size': 0x600,
             'blocks': [{'size': 0x200, 'state': 'active_allocated'}, {'size': 0x200, 'state': 'inactive'},
                        {'size': 0x200, 'state': 'active_allocated'}]},
            {'address': 0x9000, 'total_size': 0x100, 'blocks': [{'address': 0x9000, 'size': 0x100, 'state': 'inactive'}]}]
    assert _block_at(segs, 0x1000) == 'active_allocated' and _block_at(segs, 0x11ff) == 'active_allocated'
    assert _block_at(segs, 0x1200) == 'inactive' and _block_at(segs, 0x13ff) == 'inactive'
    assert _block_at(segs, 0x1400) == 'active_allocated' and _block_at(segs, 0x15ff) == 'active_allocated'
    assert _block_at(segs, 0x1600) is None and _block_at(segs, 0xfff) is None and _block_at(segs, 0x5000) is None
    assert _block_at(segs, 0x9080) == 'inactive'
    tr = [{'action': 'alloc', 'addr': 0x1200, 'size': 0x200}, {'action': 'free_requested', 'addr': 0x1200, 'size': 0x200},
          {'action': 'alloc', 'addr': 0x1200, 'size': 0x200}]
    assert _freed_after(tr, 0, 0x1234) and not _freed_after(tr, 2, 0x1234) and not _freed_after(tr, 0, 0x1400)


# ---- the reference's schedule: train, validate at another batch size (and a partial last batch), train again -------------
CASES = [('mobilenetv3_small', 'f32', None), ('mobilenetv3_large', 'f32', None), ('mobilenetv3_large', 'bf16', 'bf16'),
         ('mobilenetv2', 'f32', None)]


@pytest.mark.gpu
@pytest.mark.parametrize('name,dtype,evdt', CASES)
def test_recorded_plans_point_only_at_live_memory(name, dtype, evdt, monkeypatch):
    from torchdet3d.builders import build_loss, build_model, build_optimizer
    from torchdet3d.losses import LossManager
    from torchdet3d.trainer import Trainer, step_plan
    assert step_plan.REPLAY
    cfg = _cfg(name)
    cfg.model.storage_dtype = dtype
    cfg.model.eval_storage_dtype = evdt
    torch.manual_seed(3)
    model = build_model(cfg).to('cuda')
    model.net.reset_parameters(seed=3)
    assert (model.net_eval is model.net) == (evdt is None or evdt == dtype)
    opt = build_optimizer(cfg, model)
    lm = LossManager(build_loss(cfg), cfg.loss.coeffs, cfg.loss.alwa)
    tr = Trainer(model, None, opt, None, lm, None, 1, '', device='cuda', save_chkpt=False)
    tb, vb, vl = _batches(20, 96, nb=2), _batches(12, 96, nb=2, seed=12), _batches(5, 96, nb=1, seed=13)
    pp = PlanPointers(monkeypatch)
    it = [0]

    def plans():
        sp, fp = tr.__dict__.get('_sp'), model.__dict__.get('_fplan')
        return [sp.rec if sp else None, fp.rec if fp else None]

    def train(n):
        model.train()
        for _ in range(n):
            j = it[0] % 2
            dict(tr.train_step(tb[0][j], tb[1][j], tb[2][j], it[0]))
            it[0] += 1

    def evaluate(bs, n):
        model.eval()
        with torch.no_grad():
            for i in range(n):
                j = i % len(bs[0])
                model(bs[0][j], bs[2][j])

    try:
        train(4)
        torch.cuda.synchronize()
        assert tr._sp.rec is not None and tr._sp.replays == 1
        pp.check(plans(), 'after training at B = 20')
        evaluate(vb, 3)
        torch.cuda.synchronize()
        assert model._fplan.rec is not None and model._fplan.replays == 0
        pp.check(plans(), 'after 3 eval forwards at B = 12')
        evaluate(vl, 1)
        torch.cuda.synchronize()
        pp.check(plans(), 'after the partial eval batch B = 5')
        train(3)
        torch.cuda.synchronize()
        assert tr._sp.replays == 4
        pp.check(plans(), 'after training again at B = 20')
        evaluate(vb, 3)
        torch.cuda.synchronize()
        pp.check(plans(), 'after eval again at B = 12')
    finally:
        pp.stop()


# ---- the same loop with plans and without: bit for bit --------------------------------------------------------------------
def _main_loop(name, dtype, evdt, use_plans, pp=None):
    from torchdet3d.builders import build_loader, build_loss, build_model, build_optimizer
    from torchdet3d.evaluation import Evaluator
    from torchdet3d.losses import LossManager
    from torchdet3d.trainer import Trainer, step_plan
    from torchdet3d.utils import AttrDict
    cfg = _cfg(name)
    cfg.model.storage_dtype, cfg.model.eval_storage_dtype = dtype, evdt
    cfg.data = AttrDict(dict(root='synthetic', resize=(96, 96), train_batch_size=20, val_batch_size=12, synthetic_len=50,
                             max_epochs=3, num_workers=0))
    torch.manual_seed(7)
    model = build_model(cfg).to('cuda')
    model.net.reset_parameters(seed=7)
    opt = build_optimizer(cfg, model)
    lm = LossManager(build_loss(cfg), cfg.loss.coeffs, cfg.loss.alwa)
    train_loader, val_loader, _ = build_loader(cfg)
    assert len(val_loader.dataset) % 12 == 2
    tr = Trainer(model, train_loader, opt, None, lm, None, 3, '', device='cuda', save_chkpt=False, print_freq=1)
    ev = Evaluator(model, val_loader, cfg=cfg, device='cuda')
    if not use_plans:
        tr._sp = None

    def check(where):
        if pp is not None:
            torch.cuda.synchronize()
            sp, fp = tr.__dict__.get('_sp'), model.__dict__.get('_fplan')
            pp.check([sp.rec if sp else None, fp.rec if fp else None], where)

    def val():
        old = step_plan.REPLAY
        step_plan.REPLAY = use_plans
        try:
            return ev.val(compute_iou=True)
        finally:
            step_plan.REPLAY = old

    losses, vals = [], []
    for epoch in (0, 1):
        check(f'before epoch {epoch}')
        losses.append({k: v for k, v in tr.train(epoch, False).items() if k != 'time'})
    check('before validation 1')
    vals.append(val())
    check('before epoch 2')
    losses.append({k: v for k, v in tr.train(2, True).items() if k != 'time'})
    check('before validation 2')
    vals.append(val())
    torch.cuda.synchronize()
    st = opt.state[model.flat]
    replays = (tr._sp.replays if use_plans else 0, model._fplan.replays if use_plans else 0)
    return (model.net.flat.clone(), {k: v.clone() for k, v in model.net.buffers.items()}, st['exp_avg'].clone(),
            st['exp_avg_sq'].clone(), losses, vals, replays)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@pytest.mark.gpu
@pytest.mark.parametrize('name,dtype,evdt', [('mobilenetv3_small', 'f32', None), ('mobilenetv3_large', 'f32', None),
                                             ('mobilenetv3_small', 'bf16', 'bf16'), ('mobilenetv3_large', 'bf16', 'bf16')])
def test_replayed_training_survives_validation_at_other_batch_sizes(name, dtype, evdt, monkeypatch):
    """Model A: step plan and forward plans; model B: the eager step and launch-by-launch eval forwards.  One engine for
    training and validation in every case.  bf16 storage is bit-reproducible run to run, so A and B must agree bit for bit.
    MobileNetV3 in fp32 storage is not (DESIGN.md finding 28: fp32 atomics in the gated layers' per-sample sums, ~6e-7 run
    to run, which AdamW's normalised step turns into lr-sized moves of weights whose gradient is ~0): there the two runs
    must agree to what that noise explains (measured on MI355X: weights 2.2e-4 relative L2, epoch losses 1.9e-4, exp_avg
    2.7e-2, validation ADD / SADD / IoU 8.6e-7 -- the validation runs on the running statistics, so it is where they are
    judged; a near-zero running mean makes their own relative distance meaningless).  A plan that replays a stale
    descriptor leaves the BatchNorm sums uncleared -- batch statistics off by whole multiples, far outside every bound."""
    pp = PlanPointers(monkeypatch)
    try:
        a = _main_loop(name, dtype, evdt, True, pp)
    finally:
        pp.stop()
    b = _main_loop(name, dtype, evdt, False)
    # (two steps per epoch: epoch 0 is the two direct steps, epoch 1 records and replays, epoch 2 replays twice; each
    #  validation replays its fourth B = 12 batch)
    assert a[6] == (3, 2), a[6]
    assert any(k.endswith('num_batches_tracked') for k in b[1])
    for k in b[1]:
        if k.endswith('num_batches_tracked'):
            assert torch.equal(a[1][k], b[1][k]), k
    bn = max(_rel(a[1][k], b[1][k]) for k in b[1] if not k.endswith('num_batches_tracked'))
    dl = max(abs(x[k] - y[k]) / max(abs(y[k]), 1e-6) for x, y in zip(a[4], b[4]) for k in y if k != 'acc')
    dv = max(abs(x[k] - y[k]) for x, y in zip(a[5], b[5]) for k in y if k != 'ACC')
    print(f'[twin {name} {dtype}] weights rel L2 {_rel(a[0], b[0]):.2e}, BatchNorm buffers rel L2 {bn:.2e}, '
          f'exp_avg {_rel(a[2], b[2]):.2e}, exp_avg_sq {_rel(a[3], b[3]):.2e}, epoch losses rel {dl:.2e}, val ADD/SADD/IOU {dv:.2e}')
    if dtype == 'bf16':
        assert torch.equal(a[0], b[0]), f'weights differ: max {(a[0] - b[0]).abs().max().item():.3e}'
        for k in b[1]:
            assert torch.equal(a[1][k], b[1][k]), k
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
        assert a[4] == b[4], (a[4], b[4])
        assert a[5] == b[5], (a[5], b[5])
    else:
        assert _rel(a[0], b[0]) < 1e-3
        assert _rel(a[2], b[2]) < 1e-1 and _rel(a[3], b[3]) < 1e-1
        assert dl < 1e-3 and all(abs(x['acc'] - y['acc']) <= 0.026 for x, y in zip(a[4], b[4])), (a[4], b[4])   # (1 of 40)
        assert dv < 1e-4 and all(abs(x['ACC'] - y['ACC']) <= 0.021 for x, y in zip(a[5], b[5])), (a[5], b[5])
