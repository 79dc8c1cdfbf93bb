"""'mobilenetv3_large_21k' (the reference's default model) without a GPU: the architecture table, the builder, the
initialisation and the pretrained-checkpoint path against tests/timm_mnv3_ref.py, and that restatement against the frozen
oracle for everything but its two switches."""
import math
import socket

import pytest
import torch

import timm_mnv3_ref as R
from test_host_logic import _cfg

NAME = R.NAME


def test_parameter_count_is_the_published_one():
    shapes = R.state_dict_shapes(9)
    n = sum(math.prod(s) for k, s in shapes.items()
            if k.startswith('model.') and 'running' not in k and 'tracked' not in k)
    assert n == 4_202_032                                   # backbone: BN affine included, running stats excluded
    assert n + 1280 * 1000 + 1000 == 5_483_032              # + the removed 1000-class classifier = MobileNetV3-large-100
    heads = 9 * (18 * 1280 + 18) + 9 * 1280 + 9
    from torchdet3d.models.arch import Arch
    mine = Arch(NAME).param_shapes(9)
    assert sum(math.prod(s) for s, kind in mine.values() if kind == 'param') == n + heads
    se = [b['se'] for b in R.blocks() if b['se']]
    assert se == [24, 32, 32, 120, 168, 168, 240, 240]


@pytest.mark.parametrize('nc', [9, 1])
def test_param_shapes_equal_the_restatement(nc):
    from torchdet3d.models.arch import Arch
    mine = Arch(NAME).param_shapes(nc)
    ref = R.state_dict_shapes(nc)
    assert list(mine) == list(ref)
    assert all(tuple(mine[k][0]) == tuple(ref[k]) for k in ref)
    assert all((kind == 'buffer') == ('running' in k or 'tracked' in k) for k, (s, kind) in mine.items())


def test_gate_flag_is_per_block_and_old_names_keep_theirs():
    from torchdet3d.models.arch import Arch
    new = Arch(NAME)
    assert sum(1 for b in new.blocks if b.se) == 8 and all(b.se_after for b in new.blocks if b.se)
    assert all(b.expand for b in new.blocks if b.se)        # the gate-after path in the EXPAND layout
    assert new.head == 'conv_bias'
    for name in ('mobilenetv3_large', 'mobilenetv3_small'):
        a = Arch(name)
        assert a.head == 'linear_bn'
        assert all(b.se_after == bool(b.se and not b.expand) for b in a.blocks)


@pytest.mark.parametrize('train', [False, True])
def test_restatement_in_reference_layout_reproduces_the_oracle(train):
    """Both switches at the reference's own layout + renamed weights == oracle.model.forward('mobilenetv3_large'): pins the
    rows, channel rounding, squeeze-excite arithmetic, BatchNorm handling, heads -- everything but the two switches."""
    from oracle import model as OMod
    from oracle.weights import make_inputs, make_state_dict
    sd = make_state_dict('mobilenetv3_large', 9)
    imgs, _, cats = make_inputs(4, 96, 96, 9)
    sd_o = {k: v.clone() for k, v in sd.items()}
    sd_r = R.rename_from_reference({k: v.clone() for k, v in sd.items()})
    with torch.no_grad():
        kp_o, tg_o = OMod.forward(sd_o, 'mobilenetv3_large', imgs, cats, train=train, num_classes=9)
        kp_r, tg_r = R.forward(sd_r, imgs, cats, train=train, num_classes=9, gate_after=False, head='linear_bn')
    assert (kp_o - kp_r).abs().max().item() <= 1e-6
    assert (tg_o - tg_r).abs().max().item() <= 1e-6
    if train:        # running statistics moved alike
        assert torch.allclose(sd_o['features.4.conv.4.running_var'], sd_r['model.blocks.2.0.bn2.running_var'], atol=1e-6, rtol=0)
        assert int(sd_r['model.bn1.num_batches_tracked']) == 1


def test_each_switch_changes_the_output():
    from oracle.weights import make_inputs, make_state_dict
    sd = R.rename_from_reference(make_state_dict('mobilenetv3_large', 9))
    sd.update({k: v for k, v in R.make_state_dict(9).items() if k not in sd})
    imgs, _, cats = make_inputs(4, 96, 96, 9)
    outs = {}
    with torch.no_grad():
        for ga in (False, True):
            for head in ('linear_bn', 'conv_bias'):
                outs[ga, head] = R.forward({k: v.clone() for k, v in sd.items()}, imgs, cats, gate_after=ga, head=head)[0]
    assert (outs[False, 'linear_bn'] - outs[True, 'linear_bn']).abs().max() > 1e-4       # gate position
    assert (outs[False, 'conv_bias'] - outs[True, 'conv_bias']).abs().max() > 1e-4
    assert (outs[True, 'linear_bn'] - outs[True, 'conv_bias']).abs().max() > 1e-4        # head kind
    assert (outs[False, 'linear_bn'] - outs[False, 'conv_bias']).abs().max() > 1e-4
    # the wrapper's pool over the head's 1x1 map, kept literal: 'avg' and 'max' are the identity, 'avg+max' doubles
    sd2 = R.make_state_dict(9)
    with torch.no_grad():
        f = {m: R.pooled_features(sd2, imgs, False, pooling_mode=m) for m in ('avg', 'max', 'avg+max')}
    assert torch.equal(f['avg'], f['max']) and torch.equal(f['avg+max'], 2 * f['avg'])


def test_build_model_and_engine_construct_on_a_cpu_only_box():
    from torchdet3d.builders import AVAILABLE_MODELS, build_model
    from torchdet3d.builders.model_builder import ModelWrapper
    from torchdet3d.models.engine import Net
    assert NAME in AVAILABLE_MODELS
    m = build_model(_cfg(NAME))
    assert len(m.regressors) == 9 and m.regressors[3][0].weight.shape == (18, 1280)
    assert m.cls_fc[1].weight.shape == (9, 1280)
    assert len(list(m.parameters())) == 1
    assert list(m.state_dict()) == list(R.state_dict_shapes(9))
    for mode in ('avg', 'max', 'avg+max'):
        assert ModelWrapper(NAME, 9, pooling_mode=mode).pooling_mode == mode
    with pytest.raises(ValueError):
        ModelWrapper(NAME, 9, pooling_mode='median')
    # initialisation: conv N(0, sqrt(2 / fan_out)), fan_out = k*k*Cout / groups; zero biases; BN 1/0; heads torch's Linear default
    net = Net(NAME, 9, 'cpu')
    net.reset_parameters(seed=11)
    p = net.p
    for k, std in (('model.conv_stem.weight', (2 / (9 * 16)) ** .5), ('model.blocks.6.0.conv.weight', (2 / 960) ** .5),
                   ('model.blocks.2.0.conv_dw.weight', (2 / 25) ** .5), ('model.blocks.5.2.conv_dw.weight', (2 / 25) ** .5),
                   ('model.blocks.1.0.conv_dw.weight', (2 / 9) ** .5), ('model.blocks.5.2.conv_pwl.weight', (2 / 160) ** .5),
                   ('model.conv_head.weight', (2 / 1280) ** .5), ('model.blocks.5.0.se.conv_reduce.weight', (2 / 168) ** .5),
                   ('model.blocks.5.0.se.conv_expand.weight', (2 / 672) ** .5)):
        w = p[k]
        assert abs(w.std().item() / std - 1) < 0.12 and abs(w.mean().item()) < 4 * std / w.numel() ** .5, k
    for k, v in p.items():
        if not k.startswith('model.') or v.dim() != 1:
            continue
        assert (v == (0 if k.endswith('.bias') else 1)).all(), k          # conv / SE / BN biases 0, BN gamma 1
    b = 1 / 1280 ** .5
    for k in ('regressors.0.0.weight', 'regressors.8.0.bias', 'cls_fc.1.weight', 'cls_fc.1.bias'):
        v = p[k]
        assert v.abs().max().item() <= b and (v.numel() < 100 or abs(v.std().item() / (b / 3 ** .5) - 1) < 0.05), k
    assert all((net.buffers[k] == (1 if k.endswith('var') else 0)).all() for k in net.buffers)


def test_pretrained_loads_the_cached_timm_checkpoint_and_opens_no_socket(tmp_path, monkeypatch, capsys):
    from torchdet3d.builders import build_model

    def no_socket(*a, **k):
        raise AssertionError('model.pretrained tried to open a socket')
    monkeypatch.setattr(socket, 'socket', no_socket)
    monkeypatch.setattr(socket, 'create_connection', no_socket)
    monkeypatch.setenv('TORCH_HOME', str(tmp_path))
    cfg = _cfg(NAME)
    cfg.model.pretrained = True
    # no cached file: one line, the initialisation stays
    m0 = build_model(cfg)
    out = capsys.readouterr().out
    assert out.count('\n') == 1 and 'mobilenetv3_large_21k_imagenet.pth' in out
    assert not (m0.state_dict()['model.conv_stem.weight'] == 0.25).all()
    # a timm-format checkpoint: bare keys, conv-shaped squeeze-excite weights, a foreign classifier
    ref = R.make_state_dict(9, seed=3)
    ckpt = {k[len('model.'):]: v for k, v in ref.items() if k.startswith('model.')}
    ckpt['classifier.weight'], ckpt['classifier.bias'] = torch.zeros(1000, 1280), torch.zeros(1000)
    (tmp_path / 'checkpoints').mkdir()
    torch.save(ckpt, tmp_path / 'checkpoints' / 'mobilenetv3_large_21k_imagenet.pth')
    m = build_model(cfg)
    assert 'classifier.weight' in capsys.readouterr().out                     # reported as discarded
    got = m.state_dict()
    assert all(torch.equal(got[k], ref[k]) for k in ref if k.startswith('model.'))
    assert got['model.blocks.2.0.se.conv_reduce.weight'].shape == (24, 72, 1, 1)
    assert not torch.equal(got['regressors.0.0.weight'], ref['regressors.0.0.weight'])    # the heads keep their init
    # export mode never looks for it (model_builder.py:68), load_weights wins over it
    (tmp_path / 'checkpoints' / 'mobilenetv3_large_21k_imagenet.pth').unlink()
    build_model(cfg, export_mode=True)
    assert capsys.readouterr().out == ''
    torch.save({'state_dict': ref}, tmp_path / 'w.pth')
    cfg.model.load_weights = str(tmp_path / 'w.pth')
    m2 = build_model(cfg)
    assert torch.equal(m2.state_dict()['regressors.0.0.weight'], ref['regressors.0.0.weight'])
