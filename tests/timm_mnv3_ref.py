"""Test-side restatement of 'mobilenetv3_large_21k' (the reference's `MobileNetV3_large_100_timm` under its ModelWrapper:
torchdet3d/models/mobilenetv3.py:224-231, torchdet3d/builders/model_builder.py:73-151) as a functional
`torch.nn.functional` forward over a plain state dict -- what tests/augment_ref.py is for the augment kernel.  The frozen
oracle does not know this name, so the new tests measure the product against this file.

timm is not installed wherever this project is built or tested, so NOTHING here is pinned against timm itself: the layout
(timm's `mobilenetv3_large_100`, whose `forward_features` runs conv_stem, bn1, act1, blocks, global_pool, conv_head, act2
and returns [B,1280,1,1]) and the key names are written from knowledge of timm 0.4.x.  What IS pinned:
  * the parameter count (4 202 032 backbone parameters; + the removed 1000-class classifier's 1 281 000 = 5 483 032, the
    published size of MobileNetV3-large-100);
  * everything except the two switches below: with both set to the reference's own layout and the weights renamed
    (`rename_from_reference`), `forward` reproduces `oracle.model.forward(..., 'mobilenetv3_large', ...)`, which the goldens
    pin to the reference (tests/test_timm_mnv3_cpu.py).

The two switches (defaults = the timm layout):
  gate_after  True: every squeeze-excite gate multiplies the ACTIVATED depthwise output (dw, BN, act, SE), in both block
              layouts.  False: the reference class's positions (SE before the activation in the expand layout,
              mobilenetv3.py:155-156; after it in the other, :138-140).
  head        'conv_bias': global average pool -> conv_head (1x1, bias, no BatchNorm) -> h-swish -> the wrapper's
              `_glob_feature_vector` over the 1x1 map (model_builder.py:96-110: 'avg' and 'max' are the identity there,
              'avg+max' doubles the features).  'linear_bn': the reference class's `_glob_feature_vector` over the last
              feature map -> Linear -> BatchNorm1d -> h-swish (mobilenetv3.py:191-195), weights under
              `model.conv_head.*` (viewed as a matrix) / `model.head_bn.*`.
Any float dtype works (the state dict and the input decide); BatchNorm: eps 1e-5, momentum 0.1 (PyTorch defaults, which
timm's mobilenetv3_large_100 keeps), no dropout / stochastic depth in the backbone (timm defaults 0).
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

BN_EPS, BN_MOM = 1e-5, 0.1
NAME = 'mobilenetv3_large_21k'
# (k, t, c, SE, HS, s): the rows of the reference's model_params['mobilenetv3_large'] (mobilenetv3.py:20-36)
ROWS = [(3, 1, 16, 0, 0, 1), (3, 4, 24, 0, 0, 2), (3, 3, 24, 0, 0, 1), (5, 3, 40, 1, 0, 2), (5, 3, 40, 1, 0, 1),
        (5, 3, 40, 1, 0, 1), (3, 6, 80, 0, 1, 2), (3, 2.5, 80, 0, 1, 1), (3, 2.3, 80, 0, 1, 1), (3, 2.3, 80, 0, 1, 1),
        (3, 6, 112, 1, 1, 1), (3, 6, 112, 1, 1, 1), (5, 6, 160, 1, 1, 2), (5, 6, 160, 1, 1, 1), (5, 6, 160, 1, 1, 1)]
STAGES = (1, 2, 3, 4, 2, 3)          # blocks per timm stage; blocks.6 is the last 1x1 conv
FEAT = 1280


def make_divisible(v, divisor=8, min_value=None):
    if min_value is None:
        min_value = divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def blocks():
    out, cin = [], make_divisible(16)
    pos = [(s, j) for s, n in enumerate(STAGES) for j in range(n)]
    for (k, t, c, se, hs, s), (st, j) in zip(ROWS, pos):
        cout, cexp = make_divisible(c), make_divisible(cin * t)
        out.append(dict(p=f'model.blocks.{st}.{j}', cin=cin, cexp=cexp, cout=cout, k=k, s=s,
                        se=make_divisible(cexp * 0.25) if se else 0, act='hswish' if hs else 'relu',
                        res=(s == 1 and cin == cout)))
        cin = cout
    return out


def state_dict_shapes(num_classes=9, head='conv_bias'):
    """Ordered {key: shape}: the checkpoint surface of the model (key order = module order)."""
    out = {}

    def bn(p, c):
        out[p + '.weight'] = (c,)
        out[p + '.bias'] = (c,)
        out[p + '.running_mean'] = (c,)
        out[p + '.running_var'] = (c,)
        out[p + '.num_batches_tracked'] = ()

    out['model.conv_stem.weight'] = (16, 3, 3, 3)
    bn('model.bn1', 16)
    for b in blocks():
        p, k = b['p'], b['k']
        if b['cin'] == b['cexp']:              # timm DepthwiseSeparableConv
            out[p + '.conv_dw.weight'] = (b['cexp'], 1, k, k)
            bn(p + '.bn1', b['cexp'])
            last_w, last_bn = p + '.conv_pw.weight', p + '.bn2'
        else:                                  # timm InvertedResidual
            out[p + '.conv_pw.weight'] = (b['cexp'], b['cin'], 1, 1)
            bn(p + '.bn1', b['cexp'])
            out[p + '.conv_dw.weight'] = (b['cexp'], 1, k, k)
            bn(p + '.bn2', b['cexp'])
            last_w, last_bn = p + '.conv_pwl.weight', p + '.bn3'
        if b['se']:
            out[p + '.se.conv_reduce.weight'] = (b['se'], b['cexp'], 1, 1)
            out[p + '.se.conv_reduce.bias'] = (b['se'],)
            out[p + '.se.conv_expand.weight'] = (b['cexp'], b['se'], 1, 1)
            out[p + '.se.conv_expand.bias'] = (b['cexp'],)
        out[last_w] = (b['cout'], b['cexp'], 1, 1)
        bn(last_bn, b['cout'])
    out['model.blocks.6.0.conv.weight'] = (960, 160, 1, 1)
    bn('model.blocks.6.0.bn1', 960)
    out['model.conv_head.weight'] = (FEAT, 960, 1, 1)
    out['model.conv_head.bias'] = (FEAT,)
    if head == 'linear_bn':
        bn('model.head_bn', FEAT)
    for k in range(9):                          # always 9 heads (model_builder.py:78-81)
        out[f'regressors.{k}.0.weight'] = (18, FEAT)
        out[f'regressors.{k}.0.bias'] = (18,)
    out['cls_fc.1.weight'] = (num_classes, FEAT)
    out['cls_fc.1.bias'] = (num_classes,)
    return out


def fill(key, shape, seed=0):
    """Deterministic weight recipe in the style of oracle/weights.py: one numpy PCG64 stream per key."""
    rng = np.random.default_rng(zlib.crc32(key.encode()) + 7919 * seed)
    if key.endswith('num_batches_tracked'):
        return np.zeros((), np.int64)
    if key.endswith('running_mean'):
        return rng.uniform(-0.1, 0.1, shape).astype(np.float32)
    if key.endswith('running_var'):
        return rng.uniform(0.5, 1.5, shape).astype(np.float32)
    if len(shape) == 1 and key.endswith('.weight'):          # BN gamma
        return rng.uniform(0.5, 1.5, shape).astype(np.float32)
    if len(shape) == 1:                                        # BN beta / conv and linear biases
        return rng.uniform(-0.2, 0.2, shape).astype(np.float32)
    fan_in = int(np.prod(shape[1:]))
    a = np.sqrt(3.0 / fan_in)      # second-moment preserving: keeps eval-mode activations O(1)
    return rng.uniform(-a, a, shape).astype(np.float32)


def make_state_dict(num_classes=9, seed=0, head='conv_bias'):
    return {k: torch.from_numpy(np.array(fill(k, s, seed))) for k, s in state_dict_shapes(num_classes, head).items()}


def rename_from_reference(sd):
    """A 'mobilenetv3_large' state dict in the reference's key names (oracle.model.state_dict_shapes) -> this file's
    names, head 'linear_bn': Linear weights of the squeeze-excite FCs / the classifier become 1x1-conv shaped."""
    out = {}

    def bn(src, dst):
        for s in ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked'):
            out[f'{dst}.{s}'] = sd[f'{src}.{s}']

    out['model.conv_stem.weight'] = sd['features.0.0.weight']
    bn('features.0.1', 'model.bn1')
    for i, b in enumerate(blocks()):
        p, q = f'features.{i + 1}.conv', b['p']
        if b['cin'] == b['cexp']:
            out[q + '.conv_dw.weight'] = sd[p + '.0.weight']
            bn(p + '.1', q + '.bn1')
            se, pw, pwn, bn3, bn3n = p + '.3', p + '.4.weight', q + '.conv_pw.weight', p + '.5', q + '.bn2'
        else:
            out[q + '.conv_pw.weight'] = sd[p + '.0.weight']
            bn(p + '.1', q + '.bn1')
            out[q + '.conv_dw.weight'] = sd[p + '.3.weight']
            bn(p + '.4', q + '.bn2')
            se, pw, pwn, bn3, bn3n = p + '.5', p + '.7.weight', q + '.conv_pwl.weight', p + '.8', q + '.bn3'
        if b['se']:
            out[q + '.se.conv_reduce.weight'] = sd[se + '.fc.0.weight'][:, :, None, None]
            out[q + '.se.conv_reduce.bias'] = sd[se + '.fc.0.bias']
            out[q + '.se.conv_expand.weight'] = sd[se + '.fc.2.weight'][:, :, None, None]
            out[q + '.se.conv_expand.bias'] = sd[se + '.fc.2.bias']
        out[pwn] = sd[pw]
        bn(bn3, bn3n)
    out['model.blocks.6.0.conv.weight'] = sd['conv.0.weight']
    bn('conv.1', 'model.blocks.6.0.bn1')
    out['model.conv_head.weight'] = sd['classifier.0.weight'][:, :, None, None]
    out['model.conv_head.bias'] = sd['classifier.0.bias']
    bn('classifier.1', 'model.head_bn')
    for k, v in sd.items():
        if k.startswith(('regressors.', 'cls_fc.')):
            out[k] = v
    return out


def act_fn(x, kind):
    if kind == 'relu':
        return F.relu(x)
    if kind == 'hswish':
        return x * (F.relu6(x + 3.) / 6.)
    raise AssertionError(kind)


def hsigmoid(x):
    return F.relu6(x + 3.) / 6.


def _bn(sd, prefix, x, train):
    if train and (prefix + '.num_batches_tracked') in sd:
        sd[prefix + '.num_batches_tracked'] += 1
    return F.batch_norm(x, sd[prefix + '.running_mean'], sd[prefix + '.running_var'], sd[prefix + '.weight'],
                        sd[prefix + '.bias'], training=train, momentum=BN_MOM, eps=BN_EPS)


def _se(sd, prefix, x):
    """timm SqueezeExcite: mean over the plane -> conv_reduce -> ReLU -> conv_expand -> hard-sigmoid gate.  A 1x1 conv over
    a 1x1 map IS the matrix product with its [O,I,1,1] weight viewed as [O,I]; it is written as that product so that the
    fp32 summation order is the reference SELayer's F.linear (mobilenetv3.py:92-107) and the comparison with the oracle
    holds to 1e-6 in train mode too."""
    b, c = x.shape[:2]
    y = x.mean(dim=(2, 3))
    y = F.relu(F.linear(y, sd[prefix + '.conv_reduce.weight'].flatten(1), sd[prefix + '.conv_reduce.bias']))
    y = hsigmoid(F.linear(y, sd[prefix + '.conv_expand.weight'].flatten(1), sd[prefix + '.conv_expand.bias']))
    return x * y.view(b, c, 1, 1)


def block_forward(sd, b, x, train, gate_after):
    p, k, s, act = b['p'], b['k'], b['s'], b['act']
    y = x
    if b['cin'] == b['cexp']:
        dwbn, pw, pwbn = p + '.bn1', p + '.conv_pw.weight', p + '.bn2'
        after = True                                  # both layouts' classes gate after the activation here
    else:
        y = act_fn(_bn(sd, p + '.bn1', F.conv2d(y, sd[p + '.conv_pw.weight']), train), act)
        dwbn, pw, pwbn = p + '.bn2', p + '.conv_pwl.weight', p + '.bn3'
        after = gate_after
    y = F.conv2d(y, sd[p + '.conv_dw.weight'], None, s, (k - 1) // 2, 1, b['cexp'])
    y = _bn(sd, dwbn, y, train)
    if b['se'] and not after:
        y = _se(sd, p + '.se', y)
    y = act_fn(y, act)
    if b['se'] and after:
        y = _se(sd, p + '.se', y)
    y = _bn(sd, pwbn, F.conv2d(y, sd[pw]), train)
    return x + y if b['res'] else y


def _glob_feature_vector(x, mode):
    """model_builder.py:96-110."""
    if mode == 'avg':
        out = F.adaptive_avg_pool2d(x, 1)
    elif mode == 'max':
        out = F.adaptive_max_pool2d(x, 1)
    elif mode == 'avg+max':
        out = F.adaptive_avg_pool2d(x, 1) + F.adaptive_max_pool2d(x, 1)
    else:
        raise ValueError(f'Unknown pooling mode: {mode}')
    return out.view(x.size(0), -1)


def pooled_features(sd, x, train, gate_after=True, head='conv_bias', pooling_mode='avg'):
    y = F.conv2d(x, sd['model.conv_stem.weight'], None, 2, 1)
    y = act_fn(_bn(sd, 'model.bn1', y, train), 'hswish')
    for b in blocks():
        y = block_forward(sd, b, y, train, gate_after)
    y = act_fn(_bn(sd, 'model.blocks.6.0.bn1', F.conv2d(y, sd['model.blocks.6.0.conv.weight']), train), 'hswish')
    if head == 'conv_bias':
        y = F.adaptive_avg_pool2d(y, 1)                                   # timm's global_pool
        y = act_fn(F.conv2d(y, sd['model.conv_head.weight'], sd['model.conv_head.bias']), 'hswish')
        return _glob_feature_vector(y, pooling_mode)                      # the wrapper's pool over the 1x1 map
    f = _glob_feature_vector(y, pooling_mode)
    f = F.linear(f, sd['model.conv_head.weight'].flatten(1), sd['model.conv_head.bias'])
    return act_fn(_bn(sd, 'model.head_bn', f, train), 'hswish')


def forward(sd, x, cats, train=False, num_classes=9, dropout_mask=None, gate_after=True, head='conv_bias',
            pooling_mode='avg'):
    """ModelWrapper.forward (model_builder.py:126-146).  dropout_mask: [B,1280] tensor of {0, 2} in place of
    nn.Dropout(0.5) when train=True; None = no dropout."""
    f = pooled_features(sd, x, train, gate_after, head, pooling_mode)
    kp = torch.stack([F.linear(f[b], sd[f'regressors.{int(c)}.0.weight'], sd[f'regressors.{int(c)}.0.bias'])
                      for b, c in enumerate(cats)])
    kp = torch.sigmoid(kp).view(x.size(0), 9, 2)
    if num_classes > 1:
        fd = f * dropout_mask if (train and dropout_mask is not None) else f
        targets = F.linear(fd, sd['cls_fc.1.weight'], sd['cls_fc.1.bias'])
    else:
        targets = cats.unsqueeze(1)
    return kp, targets


def forward_to_onnx(sd, x, num_classes=9, gate_after=True, head='conv_bias', pooling_mode='avg'):
    """ModelWrapper.forward_to_onnx (model_builder.py:112-124): all 9 heads, eval."""
    f = pooled_features(sd, x, False, gate_after, head, pooling_mode)
    outs = [F.linear(f, sd[f'regressors.{k}.0.weight'], sd[f'regressors.{k}.0.bias']).view(1, x.size(0), 9, 2)
            for k in range(9)]
    kp = torch.sigmoid(torch.cat(outs))
    tg = F.linear(f, sd['cls_fc.1.weight'], sd['cls_fc.1.bias']) if num_classes > 1 else torch.zeros(x.size(0))
    return kp, tg


def cast(sd, dtype):
    """Copy of a state dict with the floating tensors in `dtype` (fp64 reference runs)."""
    return {k: (v.to(dtype) if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}
