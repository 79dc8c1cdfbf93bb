"""Backbone tables of the regression models.

mobilenetv3_{large,small}: the (k, t, c, SE, HS, s) rows, channel rounding and constructor loop
of the reference (torchdet3d/models/mobilenetv3.py:20-52 `model_params`, :54-71
`_make_divisible`, :174-188).  mobilenetv2: the standard MobileNetV2-1.0 (t, c, n, s) table
(the north-star throughput model; the reference only names it as the detector backbone,
configs/detection/mnv2_ssd_300_2_heads.py:8).

mobilenetv3_large_21k: the reference's default model (configs/default_config.py:13), its
`MobileNetV3_large_100_timm` (mobilenetv3.py:224-231): timm's `mobilenetv3_large_100` with `classifier = None`, whose
`forward_features` runs conv_stem, bn1, act1, blocks, global_pool, conv_head, act2 and returns [B,1280,1,1] (the timm
releases for which the wrapper's `output_channels=1280` / `Linear(1280, 18)` heads are self-consistent).  Same rows, channel
rounding and squeeze-excite widths as 'mobilenetv3_large'; two differences: every gate multiplies the ACTIVATED depthwise
output (also in the expand layout), and the head is global average pool -> 1x1 conv 960 -> 1280 WITH bias and WITHOUT
BatchNorm -> h-swish.  timm is not installed anywhere this project is built or tested: the layout and the key names below are
written from knowledge of timm 0.4.x and are UNPINNED against timm itself; what is pinned is the parameter count
(4 202 032 backbone parameters + the removed 1000-class classifier's 1 281 000 = 5 483 032, the published size of
MobileNetV3-large-100) and, through tests/timm_mnv3_ref.py, everything but the two differences against the reference's own
class.

State-dict key schemes (`Arch.keys`: the one table every consumer of a key name reads):

  layer                     reference class (mobilenetv3.py)        timm mobilenetv3_large_100 under `model.` (unpinned)
  stem conv / BN            features.0.0 / features.0.1             model.conv_stem / model.bn1
  block i, no expand        features.{i+1}.conv.0 dw, .1 BN,        model.blocks.S.J.conv_dw, bn1, [se], conv_pw, bn2
                            [.3 SE], .4 pw, .5 BN
  block i, expand           features.{i+1}.conv.0 pw, .1 BN, .3 dw, model.blocks.S.J.conv_pw, bn1, conv_dw, bn2, [se],
                            .4 BN, [.5 SE], .7 pw, .8 BN            conv_pwl, bn3
  squeeze-excite            <se>.fc.0 [R,C], <se>.fc.2 [C,R]        <se>.conv_reduce [R,C,1,1], <se>.conv_expand [C,R,1,1]
  last 1x1 conv / BN        conv.0 / conv.1                         model.blocks.6.0.conv / model.blocks.6.0.bn1
  head                      classifier.0 Linear, classifier.1 BN1d  model.conv_head [1280,960,1,1] + bias
  heads                     regressors.K.0, cls_fc.1                regressors.K.0, cls_fc.1
(S, J: stage and position; stages 0..5 hold 1, 2, 3, 4, 2, 3 blocks.)
"""

MOBILENETV3 = {
    'mobilenetv3_large': dict(rows=[
        (3, 1, 16, 0, 0, 1), (3, 4, 24, 0, 0, 2), (3, 3, 24, 0, 0, 1), (5, 3, 40, 1, 0, 2), (5, 3, 40, 1, 0, 1),
        (5, 3, 40, 1, 0, 1), (3, 6, 80, 0, 1, 2), (3, 2.5, 80, 0, 1, 1), (3, 2.3, 80, 0, 1, 1),
        (3, 2.3, 80, 0, 1, 1), (3, 6, 112, 1, 1, 1), (3, 6, 112, 1, 1, 1), (5, 6, 160, 1, 1, 2),
        (5, 6, 160, 1, 1, 1), (5, 6, 160, 1, 1, 1)], feat=1280),
    'mobilenetv3_small': dict(rows=[
        (3, 1, 16, 1, 0, 2), (3, 4.5, 24, 0, 0, 2), (3, 3.67, 24, 0, 0, 1), (5, 4, 40, 1, 1, 2), (5, 6, 40, 1, 1, 1),
        (5, 6, 40, 1, 1, 1), (5, 3, 48, 1, 1, 1), (5, 3, 48, 1, 1, 1), (5, 6, 96, 1, 1, 2), (5, 6, 96, 1, 1, 1),
        (5, 6, 96, 1, 1, 1)], feat=1024),
}
MOBILENETV2 = [(1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2),
               (6, 320, 1, 1)]
AVAILABLE_MODELS = ('mobilenetv2', 'mobilenetv3_large', 'mobilenetv3_small', 'mobilenetv3_large_21k', 'resnet50')
TIMM_STAGES = (1, 2, 3, 4, 2, 3)       # blocks per stage of timm's mobilenetv3_large_100 (blocks.6 is the last 1x1 conv)
# test-only name (not buildable through build_model): the reference's own `MobileNetV3(cfgs, mode='large')` class
# (mobilenetv3.py:169-197) instantiated with MobileNetV2's (t, c, n, s) table as its rows (k=3, SE=0, HS=0) -- every
# depthwise / pointwise layer from 112x112x96 on has exactly the headline model's shape, so the golden fixture generated
# from the REAL reference (oracle/gen_golden.py, tests/golden/mnv2rows_b32_224.npz) pins the benchmarked kernels' production
# shapes to the reference instead of to the oracle's restatement of MobileNetV2
MOBILENETV3['mobilenetv3_mnv2rows'] = dict(
    rows=[(3, t, c, 0, 0, s if i == 0 else 1) for t, c, n, s in MOBILENETV2 for i in range(n)], feat=1280)
TEST_ONLY_MODELS = ('resnet14', 'mobilenetv3_mnv2rows')
RESNET50_LAYERS = [(64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)]      # (width, blocks, stride of the first block)


def make_divisible(v, divisor=8, min_value=None):
    """mobilenetv3.py:54-71."""
    if min_value is None:
        min_value = divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


class Block:
    """One InvertedResidual (mobilenetv3.py:126-166)."""

    def __init__(self, cin, cexp, cout, k, s, se, act, se_after=None):
        self.cin, self.cexp, self.cout, self.k, self.s, self.se, self.act = cin, cexp, cout, k, s, se, act
        self.expand = cin != cexp            # :133 vs :146 layouts
        self.res = (s == 1 and cin == cout)  # :131
        # the gate multiplies the ACTIVATED tensor (act -> SE) instead of sitting in front of the activation (SE -> act): the
        # reference's class does that in its no-expand layout only (:138-140 against :155-156), timm in every block
        self.se_after = bool(se) and (not self.expand if se_after is None else bool(se_after))


class BlockKeys:
    """State-dict names of one block: exp_w / bn1 (None without an expansion), dw_w, bn2, se (prefix or None) with
    se_w1, se_b1 [R(,C)] and se_w2, se_b2 [C(,R)], pw_w, bn3; `first`: the block's first parameter (flat-buffer order)."""

    def __init__(self, exp_w, bn1, dw_w, bn2, se, se_fc, pw_w, bn3):
        self.exp_w, self.bn1, self.dw_w, self.bn2, self.se, self.pw_w, self.bn3 = exp_w, bn1, dw_w, bn2, se, pw_w, bn3
        if se:
            self.se_w1, self.se_b1 = f'{se}.{se_fc[0]}.weight', f'{se}.{se_fc[0]}.bias'
            self.se_w2, self.se_b2 = f'{se}.{se_fc[1]}.weight', f'{se}.{se_fc[1]}.bias'
        self.first = exp_w or dw_w


class Keys:
    """The state-dict key table of a MobileNet-layout architecture (module docstring): scheme 'reference' | 'timm'."""

    def __init__(self, arch, scheme):
        self.scheme, self.blocks = scheme, []
        if scheme == 'reference':
            self.stem_w, self.stem_bn = 'features.0.0.weight', 'features.0.1'
            for i, b in enumerate(arch.blocks):
                p = f'features.{i + 1}.conv'
                if not b.expand:
                    self.blocks.append(BlockKeys(None, None, p + '.0.weight', p + '.1', (p + '.3') if b.se else None,
                                                 ('fc.0', 'fc.2'), p + '.4.weight', p + '.5'))
                else:
                    self.blocks.append(BlockKeys(p + '.0.weight', p + '.1', p + '.3.weight', p + '.4',
                                                 (p + '.5') if b.se else None, ('fc.0', 'fc.2'), p + '.7.weight', p + '.8'))
            self.last_w, self.last_bn = 'conv.0.weight', 'conv.1'   # mobilenetv3.py:188 (`self.conv`); mobilenetv2 follows it
            self.head_w, self.head_b, self.head_bn = 'classifier.0.weight', 'classifier.0.bias', 'classifier.1'
        else:
            self.stem_w, self.stem_bn = 'model.conv_stem.weight', 'model.bn1'
            pos = [(s, j) for s, n in enumerate(TIMM_STAGES) for j in range(n)]
            assert len(pos) == len(arch.blocks)
            for (s, j), b in zip(pos, arch.blocks):
                p = f'model.blocks.{s}.{j}'
                se = (p + '.se') if b.se else None
                if not b.expand:      # timm's DepthwiseSeparableConv
                    self.blocks.append(BlockKeys(None, None, p + '.conv_dw.weight', p + '.bn1', se,
                                                 ('conv_reduce', 'conv_expand'), p + '.conv_pw.weight', p + '.bn2'))
                else:                 # timm's InvertedResidual
                    self.blocks.append(BlockKeys(p + '.conv_pw.weight', p + '.bn1', p + '.conv_dw.weight', p + '.bn2', se,
                                                 ('conv_reduce', 'conv_expand'), p + '.conv_pwl.weight', p + '.bn3'))
            self.last_w, self.last_bn = f'model.blocks.{len(TIMM_STAGES)}.0.conv.weight', f'model.blocks.{len(TIMM_STAGES)}.0.bn1'
            self.head_w, self.head_b, self.head_bn = 'model.conv_head.weight', 'model.conv_head.bias', None


class Arch:
    def __init__(self, name):
        assert name in AVAILABLE_MODELS or name in TEST_ONLY_MODELS, f'unknown model {name}'
        self.name = name
        self.blocks = []
        self.kind = 'resnet' if name in ('resnet50', 'resnet14') else 'mobilenet'
        # what sits between the pooled last feature map and the heads: None | 'linear_bn' (Linear + BatchNorm1d + h-swish,
        # mobilenetv3.py:191-195; width `classifier`) | 'conv_bias' (timm's conv_head: 1x1 conv with bias, no BatchNorm, h-swish)
        self.head = None
        if name == 'resnet14':
            # test-only: the four bottleneck kinds of ResNet-50 (projection / identity shortcut, stride 1 / 2) in a network
            # shallow enough for gradient-level comparisons (tests/test_gpu_resnet.py)
            self.layers = [(64, 2, 1), (128, 2, 2)]
            self.stem_c, self.stem_act = 64, 'relu'
            self.last_c, self.last_act, self.classifier, self.feat_c = 512, 'relu', 0, 512
        elif name == 'resnet50':
            # standard torchvision ResNet-50 (v1.5): BASELINE config 4; no reference source
            self.layers = RESNET50_LAYERS
            self.stem_c, self.stem_act = 64, 'relu'
            self.last_c, self.last_act, self.classifier, self.feat_c = 2048, 'relu', 0, 2048
        elif name == 'mobilenetv2':
            self.stem_c, self.stem_act = 32, 'relu6'
            cin = 32
            for t, c, n, s in MOBILENETV2:
                for i in range(n):
                    self.blocks.append(Block(cin, cin * t, c, 3, s if i == 0 else 1, 0, 'relu6'))
                    cin = c
            self.last_c, self.last_act, self.classifier, self.feat_c = 1280, 'relu6', 0, 1280
        else:
            timm = name == 'mobilenetv3_large_21k'
            spec = MOBILENETV3['mobilenetv3_large' if timm else name]
            self.stem_c, self.stem_act = make_divisible(16), 'hswish'
            cin = self.stem_c
            cexp = cin
            for k, t, c, se, hs, s in spec['rows']:
                cout = make_divisible(c)
                cexp = make_divisible(cin * t)
                self.blocks.append(Block(cin, cexp, cout, k, s, make_divisible(cexp // 4) if se else 0,
                                         'hswish' if hs else 'relu', se_after=True if timm else None))
                cin = cout
            self.last_c, self.last_act = cexp, 'hswish'
            self.classifier = self.feat_c = spec['feat']
            self.head = 'conv_bias' if timm else 'linear_bn'
        if self.kind == 'mobilenet':
            self.keys = Keys(self, 'timm' if name == 'mobilenetv3_large_21k' else 'reference')

    def param_shapes(self, num_classes):
        """Ordered {state-dict key: (shape, kind)}; kind in param | buffer.  Key names and order are the
        reference's (`state_dict()` of ModelWrapper(MobileNetV3))."""
        out = {}
        if self.kind == 'resnet':
            return self._resnet_shapes(num_classes)

        def bn(p, c):
            out[p + '.weight'] = ((c,), 'param')
            out[p + '.bias'] = ((c,), 'param')
            out[p + '.running_mean'] = ((c,), 'buffer')
            out[p + '.running_var'] = ((c,), 'buffer')
            out[p + '.num_batches_tracked'] = ((), 'buffer')

        K = self.keys
        conv_se = K.scheme == 'timm'          # timm's SqueezeExcite holds 1x1 convs, the reference's SELayer Linears

        def se(bk, c, h):
            out[bk.se_w1] = ((h, c, 1, 1) if conv_se else (h, c), 'param')
            out[bk.se_b1] = ((h,), 'param')
            out[bk.se_w2] = ((c, h, 1, 1) if conv_se else (c, h), 'param')
            out[bk.se_b2] = ((c,), 'param')

        out[K.stem_w] = ((self.stem_c, 3, 3, 3), 'param')
        bn(K.stem_bn, self.stem_c)
        for b, bk in zip(self.blocks, K.blocks):
            if b.expand:
                out[bk.exp_w] = ((b.cexp, b.cin, 1, 1), 'param')
                bn(bk.bn1, b.cexp)
            out[bk.dw_w] = ((b.cexp, 1, b.k, b.k), 'param')
            bn(bk.bn2, b.cexp)
            if b.se:
                se(bk, b.cexp, b.se)
            out[bk.pw_w] = ((b.cout, b.cexp, 1, 1), 'param')
            bn(bk.bn3, b.cout)
        out[K.last_w] = ((self.last_c, self.blocks[-1].cout, 1, 1), 'param')
        bn(K.last_bn, self.last_c)
        if self.head == 'linear_bn':
            out[K.head_w] = ((self.classifier, self.last_c), 'param')
            out[K.head_b] = ((self.classifier,), 'param')
            bn(K.head_bn, self.classifier)
        elif self.head == 'conv_bias':
            out[K.head_w] = ((self.classifier, self.last_c, 1, 1), 'param')
            out[K.head_b] = ((self.classifier,), 'param')
        for k in range(9):                                   # always 9 heads (model_builder.py:78-81)
            out[f'regressors.{k}.0.weight'] = ((18, self.feat_c), 'param')
            out[f'regressors.{k}.0.bias'] = ((18,), 'param')
        out['cls_fc.1.weight'] = ((num_classes, self.feat_c), 'param')
        out['cls_fc.1.bias'] = ((num_classes,), 'param')
        return out

    def _resnet_shapes(self, num_classes):
        """torchvision's ResNet-50 state-dict keys + the wrapper's heads (model_builder.py:79-85)."""
        out = {}

        def bn(p, c):
            out[p + '.weight'] = ((c,), 'param')
            out[p + '.bias'] = ((c,), 'param')
            out[p + '.running_mean'] = ((c,), 'buffer')
            out[p + '.running_var'] = ((c,), 'buffer')
            out[p + '.num_batches_tracked'] = ((), 'buffer')
        out['conv1.weight'] = ((64, 3, 7, 7), 'param')
        bn('bn1', 64)
        cin = 64
        for li, (w, n, s) in enumerate(self.layers):
            for i in range(n):
                p = f'layer{li + 1}.{i}'
                out[p + '.conv1.weight'] = ((w, cin, 1, 1), 'param')
                bn(p + '.bn1', w)
                out[p + '.conv2.weight'] = ((w, w, 3, 3), 'param')
                bn(p + '.bn2', w)
                out[p + '.conv3.weight'] = ((4 * w, w, 1, 1), 'param')
                bn(p + '.bn3', 4 * w)
                if i == 0:
                    out[p + '.downsample.0.weight'] = ((4 * w, cin, 1, 1), 'param')
                    bn(p + '.downsample.1', 4 * w)
                cin = 4 * w
        for k in range(9):
            out[f'regressors.{k}.0.weight'] = ((18, self.feat_c), 'param')
            out[f'regressors.{k}.0.bias'] = ((18,), 'param')
        out['cls_fc.1.weight'] = ((num_classes, self.feat_c), 'param')
        out['cls_fc.1.bias'] = ((num_classes,), 'param')
        return out
