"""SSD300-MobileNetV2 detector of the two-stage pipeline (BASELINE config 5), inference, on the HIP path.

What the reference holds of it is the mmdetection CONFIG (`configs/detection/mnv2_ssd_300_2_heads.py`: backbone
`mobilenetv2_w1` tapped at its 96- and 320-channel maps :7-13, `SSDHead` with depthwise heads + ReLU :15-37, clustered
anchors of strides 16 / 32 :19-31, DeltaXYWH coder with stds (0.1, 0.1, 0.2, 0.2) :32-35, test_cfg score 0.02 / NMS 0.45 /
200 per image :65-69) and the OpenVINO wrapper that runs the exported IR (`torchdet3d/utils/ie_wrappers.py:70-120`); the
model code lives in an external mmdetection fork (README.md:56-57).  So the arithmetic here follows the PUBLISHED mmdet
definitions of those config entries and is restated in oracle/ssd.py -- **parity with the reference's detector is
unpinned** (no source, no weights); the layers themselves are the product's own kernels:
  backbone   models.engine.Net('mobilenetv2') in inference mode, tapped after features.13 (96 ch, stride 16) and
             features.17 (320 ch, stride 32)
  heads      per level and branch: depthwise 3x3 (t3d_dwconv_fwd) -> BatchNorm + ReLU applied on load by the 1x1 conv
             with bias (t3d_pwconv_fwd); class branch A*(classes+1) channels (background last), box branch A*4
  post       t3d_ssd_decode_nms: decode + softmax + per-class NMS in one launch; the overall top-`max_per_img` on the host
             (`detect`) or on the device (`detect_device` + t3d_ssd_select_rects: utils/pipeline.py)
  loss       `loss`: the config's training half :41-55 (targets, MultiBox loss, gradients with respect to the head outputs)
             through t3d_ssd_multibox_loss (losses/detection_losses.py).
  data       the config's train / test pipelines :63-143 on whole frames: `builders.build_detection_loader(cfg)` ->
             `GpuDetectionLoader` (dataloaders/detection.py, gpu_detection_loader.py; one t3d_detect_augment_u8 launch per
             batch), which yields exactly the (imgs, gt_boxes, gt_labels, gt_counts) `loss` takes and the uint8 frames `detect`
             takes.
  training   piece (b1), the heads: `head_backward` runs the heads with train-mode BatchNorm over the FROZEN backbone
             (inference mode, running statistics, nothing of it changes), the MultiBox loss, t3d_ssd_head_bwd (the 1x1 half
             of every head in one call, on the loss's fp32 gradients), t3d_bn_bwd_finalize and t3d_dwconv_bwd; the parameter
             gradients land in the flat buffer `hgrad` (same layout as the parameters' `hflat`), the gradients at the two
             taps come out on request.  `trainer.DetectorHeadTrainer` steps `hflat` with the config's SGD :145-153.
             Piece (b2), the backbone: `train_backward` runs the tapped backbone in training mode
             (`Net.forward_taps_train`), the same head half, and sends the tap gradients through `Net.backward_taps` -- the
             middle tap joins as the residual of features.14's expansion data gradient, the deepest one enters through a
             t3d_bn_act_bwd seed launch; `trainer.DetectorTrainer` steps `hflat` and the backbone's trained prefix of `flat`.
"""
import ctypes
import math

import numpy as np
import torch

from .. import _native as N
from .engine import DW_SLOTS, Net

INPUT_SIZE = 300
CLASSES = ('bike', 'book', 'bottle', 'camera', 'cereal_box', 'chair', 'cup', 'laptop', 'shoe')     # config :4
STRIDES = (16, 32)
WIDTHS = ([0.2579684384230685, 0.4627705986569778, 0.34682129636083536, 0.641596163690939],
          [0.5420266488537757, 0.430022826081911, 0.7605568897973095, 0.6358004294180672, 0.5529565428117278,
           0.8008912664437589])                                                                     # config :21-25 (x input_size)
HEIGHTS = ([0.2270640055663951, 0.30064816327707244, 0.4627093933691148, 0.33801734483143625],
           [0.47856221526606557, 0.6557960498140745, 0.49101025166070583, 0.6256796503549162, 0.8331586024284066,
            0.7244268959927074])                                                                    # config :26-31
STDS = (0.1, 0.1, 0.2, 0.2)                                                                         # config :34
TAPS = (13, 17)                  # features.13 -> 96 channels @ stride 16, features.17 -> 320 channels @ stride 32
TAP_CHANNELS = (96, 320)
BN_EPS = 1e-5
BN_MOMENTUM = 0.1
BRANCHES = ('cls_convs', 'reg_convs')


def make_anchors(input_size=INPUT_SIZE):
    """[sum_l H_l*W_l*A_l, 4] (x1, y1, x2, y2), level-major, then pixel (row-major), then anchor: boxes of the clustered
    widths / heights centred on the cell centres stride*(i + 0.5)."""
    out = []
    for l, s in enumerate(STRIDES):
        fm = math.ceil(input_size / s)
        cy, cx = np.meshgrid((np.arange(fm) + 0.5) * s, (np.arange(fm) + 0.5) * s, indexing='ij')
        w, h = np.asarray(WIDTHS[l]) * input_size, np.asarray(HEIGHTS[l]) * input_size
        a = np.stack([cx[..., None] - w / 2, cy[..., None] - h / 2, cx[..., None] + w / 2, cy[..., None] + h / 2], -1)
        out.append(a.reshape(-1, 4))
    return np.concatenate(out).astype(np.float32)


def head_param_shapes(num_classes=len(CLASSES)):
    """State-dict entries of the SSD head (mmdet's SSDHead with depthwise_heads: Sequential(dw conv, BN, ReLU, 1x1 conv))."""
    out = {}
    for l, C in enumerate(TAP_CHANNELS):
        A = len(WIDTHS[l])
        for br, n in (('cls_convs', A * (num_classes + 1)), ('reg_convs', A * 4)):
            p = f'bbox_head.{br}.{l}'
            out[p + '.0.weight'] = (C, 1, 3, 3)
            for k, shp in (('weight', (C,)), ('bias', (C,)), ('running_mean', (C,)), ('running_var', (C,))):
                out[f'{p}.1.{k}'] = shp
            out[p + '.3.weight'] = (n, C, 1, 1)
            out[p + '.3.bias'] = (n,)
    return out


def flat_head_layout(num_classes=len(CLASSES)):
    """{learnable state-dict entry: (offset, reserved elements)} in the flat parameter / gradient buffers.  A 1x1 conv's weight
    and bias reserve their rows padded to a multiple of 8 -- the matrix and bias the kernels read --; the pad stays zero
    (zero parameter, zero gradient: SGD with weight decay leaves it there).  Every offset is a multiple of 4 elements."""
    out, off = {}, 0
    for k, shp in head_param_shapes(num_classes).items():
        if 'running' in k:
            continue
        n = int(np.prod(shp))
        if '.3.' in k:
            n = (shp[0] + 7) // 8 * 8 * (n // shp[0])
        n = (n + 3) // 4 * 4
        out[k] = (off, n)
        off += n
    return out


class SSD300:
    """`detect(frames_u8)` -> per image an [n, 6] array (x1, y1, x2, y2 normalised to [0, 1], score, label)."""

    # config :41-55: the assigner's thresholds and the head's loss settings (the entries this project builds; the same lines'
    # `loss_balancing=True` is the fork's own learnable weighting, has no published definition and is not built)
    TRAIN_CFG = dict(pos_iou_thr=0.4, neg_iou_thr=0.4, min_pos_iou=0., gt_max_assign_all=False, smoothl1_beta=1.,
                     neg_pos_ratio=3)

    def __init__(self, device='cuda', dtype=torch.bfloat16, num_classes=len(CLASSES), score_thr=0.02, iou_thr=0.45,
                 max_per_img=200, seed=0):
        self.device, self.dtype, self.nc = torch.device(device), dtype, num_classes
        self.dt = N.F32 if dtype == torch.float32 else N.BF16
        self.score_thr, self.iou_thr, self.max_per_img = score_thr, iou_thr, max_per_img
        self.backbone = Net('mobilenetv2', 9, device, dtype)        # (the regression heads of the engine stay unused)
        self.backbone.reset_parameters(seed=seed)
        self.anchors = torch.from_numpy(make_anchors()).to(self.device)
        g = torch.Generator().manual_seed(seed + 1)
        # the learnable head parameters are views on ONE flat fp32 buffer (what t3d_sgd_step steps), their gradients views on
        # `hgrad` of the same layout; the running statistics are tensors of their own
        shapes = head_param_shapes(num_classes)
        self.hlayout = flat_head_layout(num_classes)
        total = max(o + n for o, n in self.hlayout.values())
        self.hflat = torch.zeros((total + 3) // 4 * 4, device=self.device)
        self.hgrad = torch.zeros_like(self.hflat)
        self.p, self.hg = {}, {}
        for k, shp in shapes.items():
            if k.endswith('running_var') or k.endswith('.1.weight'):
                v = torch.ones(shp)
            elif k.endswith('.0.weight') or k.endswith('.3.weight'):
                fan = shp[1] * shp[2] * shp[3]
                v = torch.randn(shp, generator=g) * math.sqrt(2.0 / fan)
            else:
                v = torch.zeros(shp)
            if k in self.hlayout:
                o, n = self.hlayout[k][0], v.numel()
                self.p[k] = self.hflat[o:o + n].view(shp)
                self.hg[k] = self.hgrad[o:o + n].view(shp)
                self.p[k].copy_(v)
            else:
                self.p[k] = v.to(self.device)
        self._packed = None
        self._train = {}
        self._stds = (ctypes.c_float * 4)(*STDS)
        self._persist, self._hbufs, self._dev = False, {}, {}
        self._mbox = None

    def state_dict(self):
        sd = {'backbone.' + k: v for k, v in self.backbone.state_dict().items()
              if not (k.startswith('regressors') or k.startswith('cls_fc'))}
        sd.update({k: v.detach().clone() for k, v in self.p.items()})
        return sd

    def load_state_dict(self, sd):
        bb = self.backbone.state_dict()
        bb.update({k[len('backbone.'):]: v for k, v in sd.items() if k.startswith('backbone.')})
        self.backbone.load_state_dict(bb)
        for k in self.p:
            self.p[k].copy_(torch.as_tensor(sd[k]).to(self.device).view(self.p[k].shape))
        self.params_changed()

    def params_changed(self):
        """After any change of the head parameters or running statistics: the eval-mode path folds the new values on its next
        call, the training path repacks its 1x1 weights."""
        self._packed = None
        for s in self._train.values():
            s['stale'] = True

    def _pack(self):
        """1x1 weights in the storage dtype, output channels padded to a multiple of 8 (zero rows); BatchNorm folded to the
        per-channel affine the 1x1 conv applies on load."""
        packed = []
        for l, C in enumerate(TAP_CHANNELS):
            lv = {}
            for br in ('cls_convs', 'reg_convs'):
                p = f'bbox_head.{br}.{l}'
                w = self.p[p + '.3.weight'].view(-1, C)
                n = w.shape[0]
                npad = (n + 7) // 8 * 8
                wp = torch.zeros(npad, C, device=self.device)
                wp[:n] = w
                bp = torch.zeros(npad, device=self.device)
                bp[:n] = self.p[p + '.3.bias']
                scale, shift = torch.empty(C, device=self.device), torch.empty(C, device=self.device)
                N.call('t3d_bn_eval_affine', C, N.ptr(self.p[p + '.1.weight']), N.ptr(self.p[p + '.1.bias']),
                       N.ptr(self.p[p + '.1.running_mean']), N.ptr(self.p[p + '.1.running_var']), BN_EPS, N.ptr(scale),
                       N.ptr(shift), N.stream())
                lv[br] = dict(wdw=self.p[p + '.0.weight'].view(C, 9).contiguous(), w=wp.to(self.dtype).contiguous(), b=bp,
                              pro=N.prologue(scale, shift, None, 'relu', False), n=npad)
            packed.append(lv)
        self._packed = packed

    def _hbuf(self, key, shape):
        """Head activation buffer: fresh per call, or -- inside `detect_device`, whose chain a plan may replay -- one
        persistent tensor per (level, branch, shape)."""
        if not self._persist:
            return torch.empty(shape, device=self.device, dtype=self.dtype)
        t = self._hbufs.get((key, shape))
        if t is None:
            t = self._hbufs[(key, shape)] = torch.empty(shape, device=self.device, dtype=self.dtype)
        return t

    @torch.no_grad()
    def head_outputs(self, imgs):
        """imgs: uint8 NHWC [B,300,300,3] (normalised in the stem) or fp32 NCHW -> per level (cls [B*HW, n_cls], reg
        [B*HW, n_reg], HW)."""
        if self._packed is None:
            self._pack()
        taps = self.backbone.forward_taps(imgs, TAPS)
        st, outs = N.stream(), []
        for l, k in enumerate(TAPS):
            t, B, H, W, C = taps[k]
            lv, res = self._packed[l], []
            for br in ('cls_convs', 'reg_convs'):
                h = lv[br]
                y = self._hbuf((l, br, 'y'), (B * H * W, C))
                N.call('t3d_dwconv_fwd', self.dt, N.ptr(t), None, N.ptr(h['wdw']), N.ptr(y), None, None, B, H, W, C, 3, 1, st)
                o = self._hbuf((l, br, 'o'), (B * H * W, h['n']))
                N.call('t3d_pwconv_fwd', self.dt, N.ptr(y), h['pro'], N.ptr(h['w']), N.ptr(h['b']), N.ptr(o), None,
                       B * H * W, H * W, C, h['n'], st)
                res.append(o)
            outs.append((res[0], res[1], H * W))
        return outs

    @torch.no_grad()
    def loss(self, imgs, gt_boxes, gt_labels, gt_counts, with_grads=False):
        """`head_outputs` (BatchNorm in eval mode, as everywhere in this class) followed by the MultiBox loss of TRAIN_CFG:
        gt_boxes [B,G,4] fp32 in input pixels, gt_labels [B,G] int32, gt_counts [B] int32 -> `MultiBoxLoss.from_heads`'
        dict (the validation loss of the loaded checkpoint; with `with_grads` the gradients with respect to the head
        outputs, which a backward through the heads would consume).  Nothing is synchronised."""
        outs = self.head_outputs(imgs)
        return self._multibox().from_heads(outs, gt_boxes, gt_labels, gt_counts, with_grads=with_grads,
                                           nanchors=[len(WIDTHS[l]) for l in range(len(outs))])

    def _multibox(self):
        if self._mbox is None:
            from ..losses.detection_losses import MultiBoxLoss
            t = self.TRAIN_CFG
            self._mbox = MultiBoxLoss(self.anchors, self.nc, t['pos_iou_thr'], t['neg_iou_thr'], t['min_pos_iou'],
                                      t['neg_pos_ratio'], t['smoothl1_beta'], STDS)
        return self._mbox

    # ------------------------------------------------------------------ training-mode heads (piece b1)
    def _train_state(self, B, dims):
        """The persistent buffers of `head_backward` at batch size B (a recorded plan points into them): per head the raw
        depthwise output, the head output, the gradient at the BatchNorm output, the tap gradient, the BatchNorm's sums and
        coefficients, the depthwise weight-gradient slots; and the host arrays t3d_ssd_head_bwd takes."""
        s = self._train.get(B)
        if s is not None:
            return s
        dev, f32 = self.device, torch.float32
        heads = []
        for l, (H, W, C) in enumerate(dims):
            M = B * H * W
            for br in BRANCHES:
                p = f'bbox_head.{br}.{l}'
                n = self.p[p + '.3.bias'].shape[0]
                npad = (n + 7) // 8 * 8
                o, _ = self.hlayout[p + '.3.weight']
                ob, _ = self.hlayout[p + '.3.bias']
                h = dict(l=l, br=br, p=p, M=M, H=H, W=W, C=C, n=n, ns=npad,
                         w32=self.hflat[o:o + npad * C].view(npad, C), bias=self.hflat[ob:ob + npad],
                         w=torch.zeros(npad, C, device=dev, dtype=self.dtype),
                         y=torch.empty(M, C, device=dev, dtype=self.dtype), o=torch.empty(M, npad, device=dev, dtype=self.dtype),
                         g=torch.empty(M, C, device=dev, dtype=self.dtype), dx=torch.empty(M, C, device=dev, dtype=self.dtype),
                         coef=torch.zeros(7, C, device=dev, dtype=f32),      # scale, shift, mean, invstd, alpha, beta, gammac
                         slots=torch.zeros(DW_SLOTS, C * 9, device=dev, dtype=f32))
                h['pro'] = N.prologue(h['coef'][0], h['coef'][1], None, 'relu', False)
                h['bb'] = N.bnbwd(h['coef'][4], h['coef'][5], h['coef'][6], False)
                heads.append(h)
        nh = len(heads)
        # forward sums | backward sums of every head: one zero fill
        offs = np.cumsum([0] + [4 * h['C'] for h in heads])
        sums = torch.zeros(int(offs[-1]), device=dev, dtype=torch.float64)
        used = torch.zeros(nh, device=dev, dtype=torch.int32)
        for i, h in enumerate(heads):
            h['stats'], h['bstats'] = sums[offs[i]:offs[i] + 2 * h['C']], sums[offs[i] + 2 * h['C']:offs[i + 1]]
            h['used'] = used[i:i + 1]
        P, I = ctypes.c_void_p * nh, ctypes.c_int * nh
        geo = [I(*[h[k] for h in heads]) for k in ('M', 'C', 'n', 'ns')]
        nb = N.lib().t3d_ssd_head_bwd_work_bytes(nh, *[ctypes.addressof(a) for a in geo[:3]])
        if nb < 0:
            raise RuntimeError(f't3d_ssd_head_bwd_work_bytes failed with code {nb}')
        s = dict(heads=heads, sums=sums, used=used, geo=geo, work=torch.empty(nb // 8 + 1, device=dev, dtype=torch.float64), nb=nb,
                 zero=torch.tensor([[sums.data_ptr(), sums.numel() * 8]], dtype=torch.int64, device=dev),
                 pack=torch.tensor([[h['w32'].data_ptr(), h['w'].data_ptr(), 0, h['ns'], h['C'], 0, 0] for h in heads],
                                   dtype=torch.int64, device=dev),
                 flush=torch.tensor([[h['slots'].data_ptr(), self.hg[h['p'] + '.0.weight'].data_ptr(), h['C'] * 9,
                                      h['used'].data_ptr()] for h in heads], dtype=torch.int64, device=dev),
                 # (the loss's gradient pointers are filled in per call: `from_heads` allocates them)
                 ptrs={k: P(*[t.data_ptr() for t in ts]) for k, ts in dict(
                     y=[h['y'] for h in heads], scale=[h['coef'][0] for h in heads], shift=[h['coef'][1] for h in heads],
                     w=[h['w'] for h in heads], g=[h['g'] for h in heads], stats=[h['bstats'] for h in heads],
                     dW=[self.hg[h['p'] + '.3.weight'] for h in heads], dbias=[self.hg[h['p'] + '.3.bias'] for h in heads]).items()},
                 P=P, stale=True)
        self._train[B] = s
        return s

    def repack_heads(self, B=None):
        """The heads' 1x1 weights in the storage dtype from `hflat`, every head in one launch (after an optimizer step)."""
        for s in ([self._train[B]] if B is not None else self._train.values()):
            N.call('t3d_pack_weights_batched', self.dt, N.ptr(s['pack']), s['pack'].shape[0], N.stream())
            s['stale'] = False

    @torch.no_grad()
    def head_backward(self, imgs, gt_boxes, gt_labels, gt_counts, tap_grads=False):
        """One training forward + backward of the four heads over the FROZEN backbone (the taps come from `forward_taps`:
        inference mode, nothing of `self.backbone` changes).  The head BatchNorms run in training mode (the config's
        norm_eval=False): batch statistics of count B*H*W, momentum 0.1, the running estimates updated with the unbiased
        variance.  -> the dict of `MultiBoxLoss.from_heads` plus `dtaps`: with `tap_grads` the gradient at each tap
        [B*H*W, C] in the storage dtype, class and box branch summed (else None).  The parameter gradients are left in
        `hgrad` (views: `hg`).  Nothing is synchronised and every launch goes through `N.call`."""
        return self._heads_fwd_bwd(self.backbone.forward_taps(imgs, TAPS), int(imgs.shape[0]), gt_boxes, gt_labels, gt_counts,
                                   tap_grads)

    def _heads_fwd_bwd(self, taps, B, gt_boxes, gt_labels, gt_counts, tap_grads):
        """The head half of `head_backward` / `train_backward` on given taps (the dict of `Net.forward_taps`)."""
        s = self._train_state(B, [taps[k][2:5] for k in TAPS])
        st, heads, rec = N.stream(), s['heads'], N.recorder
        if rec is not None:
            rec.keep.append(s)
        if s['stale'] or rec is not None:
            self.repack_heads(B)
        N.call('t3d_set_reduction_replicas', 1, 0)
        N.call('t3d_zero_batched', N.ptr(s['zero']), 1, st)
        # ---- forward: depthwise conv + batch sums -> affine (running estimates move) -> ReLU + 1x1 conv with bias
        for h in heads:
            t, M, H, W, C, c = taps[TAPS[h['l']]][0], h['M'], h['H'], h['W'], h['C'], h['coef']
            p = h['p']
            N.call('t3d_dwconv_fwd', self.dt, N.ptr(t), None, N.ptr(self.p[p + '.0.weight']), N.ptr(h['y']), N.ptr(h['stats']),
                   None, B, H, W, C, 3, 1, st)
            N.call('t3d_bn_finalize', N.ptr(h['stats']), C, float(M), N.ptr(self.p[p + '.1.weight']), N.ptr(self.p[p + '.1.bias']),
                   N.ptr(self.p[p + '.1.running_mean']), N.ptr(self.p[p + '.1.running_var']), None, BN_MOMENTUM, BN_EPS,
                   N.ptr(c[0]), N.ptr(c[1]), N.ptr(c[2]), N.ptr(c[3]), st)
            N.call('t3d_pwconv_fwd', self.dt, N.ptr(h['y']), h['pro'], N.ptr(h['w']), N.ptr(h['bias']), N.ptr(h['o']), None,
                   M, H * W, C, h['ns'], st)
        self._packed = None           # (the running statistics moved: the eval path folds them again)
        outs = [(heads[2 * l]['o'], heads[2 * l + 1]['o'], heads[2 * l]['H'] * heads[2 * l]['W']) for l in range(len(TAPS))]
        r = self._multibox().from_heads(outs, gt_boxes, gt_labels, gt_counts, with_grads=True,
                                        nanchors=[len(WIDTHS[l]) for l in range(len(TAPS))])
        # ---- backward of the 1x1 half, every head in one call, on the loss's fp32 gradients
        dout = s['P'](*[r['grads'][h['l']][BRANCHES.index(h['br'])].data_ptr() for h in heads])
        if rec is not None:
            rec.keep += [dout, r]
        a = lambda x: ctypes.addressof(x)
        pt = s['ptrs']
        N.call('t3d_ssd_head_bwd', self.dt, len(heads), a(dout), a(pt['y']), a(pt['scale']), a(pt['shift']), a(pt['w']),
               *[a(x) for x in s['geo']], N.ACT['relu'], a(pt['g']), a(pt['stats']), a(pt['dW']), a(pt['dbias']),
               N.ptr(s['work']), s['nb'], st)
        s['dout'] = dout              # (alive until the next call: the entry point reads the array before it returns)
        # ---- BatchNorm backward -> dgamma, dbeta and the affine the depthwise backward applies; depthwise backward
        dtaps = []
        for i, h in enumerate(heads):
            t, M, H, W, C, c = taps[TAPS[h['l']]][0], h['M'], h['H'], h['W'], h['C'], h['coef']
            p = h['p']
            N.call('t3d_bn_bwd_finalize', N.ptr(h['bstats']), C, float(M), N.ptr(self.p[p + '.1.weight']), N.ptr(c[2]), N.ptr(c[3]),
                   N.ptr(c[4]), N.ptr(c[5]), N.ptr(c[6]), N.ptr(self.hg[p + '.1.weight']), N.ptr(self.hg[p + '.1.bias']), st)
            N.call('t3d_set_dw_slots', DW_SLOTS, N.ptr(h['used']))
            # (the entry point needs a dx buffer either way; the class branch's result is the box branch's `residual`)
            res = heads[i - 1]['dx'] if (tap_grads and h['br'] == BRANCHES[1]) else None
            N.call('t3d_dwconv_bwd', self.dt, N.ptr(h['g']), N.ptr(h['y']), h['bb'], N.ptr(self.p[p + '.0.weight']), N.ptr(t),
                   None, N.ptr(res), N.ptr(h['dx']), None, N.ptr(h['slots']), B, H, W, C, 3, 1, st)
            if tap_grads and h['br'] == BRANCHES[1]:
                dtaps.append(h['dx'])
        N.call('t3d_set_dw_slots', 0, None)
        N.call('t3d_sum_slots_batched', N.ptr(s['flush']), len(heads), st)
        r = dict(r)
        r['dtaps'] = dtaps if tap_grads else None
        return r

    @torch.no_grad()
    def train_backward(self, imgs, gt_boxes, gt_labels, gt_counts):
        """One training forward + backward of the WHOLE detector (piece (b2); the config's norm_eval=False,
        frozen_stages=-1): the tapped backbone in training mode (`Net.forward_taps_train`: batch statistics, running
        estimates moved), the head half of `head_backward` on those taps, and the tap gradients sent back through
        `Net.backward_taps`.  Head gradients land in `hgrad`, backbone gradients in `backbone.gflat` (zero outside the stem
        and features.*).  -> the dict of `head_backward` with the tap gradients.  Nothing is synchronised and every launch
        goes through `N.call`."""
        bb = self.backbone
        taps = bb.forward_taps_train(imgs, TAPS)
        # (the engine's pass has settled every BatchNorm the taps were read through and left the library's process-wide state
        # at its defaults, which is what the head half starts from; `backward_taps` sets its own again)
        r = self._heads_fwd_bwd(taps, int(imgs.shape[0]), gt_boxes, gt_labels, gt_counts, True)
        bb.backward_taps(dict(zip(TAPS, r['dtaps'])))
        return r

    @torch.no_grad()
    def detect_device(self, imgs):
        """The detector's launch chain with nothing read back: -> (out [B,nc,K,6] fp32: x1, y1, x2, y2 in input pixels, score,
        label per class in NMS order; cnt [B,nc] int32 valid rows) on the device, in buffers that persist per batch size
        (valid until the next call at that batch size; rows past cnt are stale -- the decode kernel writes every count and
        the rows below it, so nothing needs clearing)."""
        self._persist = True
        try:
            outs = self.head_outputs(imgs)
        finally:
            self._persist = False
        B = int(imgs.shape[0])
        nl = len(outs)
        K = self.max_per_img
        d = self._dev.get(B)
        if d is None:
            d = self._dev[B] = dict(out=torch.zeros(B, self.nc, K, 6, device=self.device),
                                    cnt=torch.zeros(B, self.nc, dtype=torch.int32, device=self.device))
        P, I = ctypes.c_void_p * nl, ctypes.c_int * nl
        # the per-level HOST arrays the entry point takes; handed over as addresses, which a recorded plan keeps as they are
        host = (P(*[o[0].data_ptr() for o in outs]), P(*[o[1].data_ptr() for o in outs]), I(*[o[2] for o in outs]),
                I(*[len(WIDTHS[l]) for l in range(nl)]), I(*[o[0].shape[1] for o in outs]), I(*[o[1].shape[1] for o in outs]))
        d['host'] = host
        if N.recorder is not None:
            N.recorder.keep += [host, self._stds, outs, d['out'], d['cnt'], self.anchors]
        N.call('t3d_ssd_decode_nms', self.dt, nl, *[ctypes.addressof(h) for h in host], N.ptr(self.anchors), B, self.nc,
               float(self.score_thr), float(self.iou_thr), K, float(INPUT_SIZE), float(INPUT_SIZE),
               ctypes.addressof(self._stds), N.ptr(d['out']), N.ptr(d['cnt']), N.stream())
        return d['out'], d['cnt']

    @staticmethod
    def merge_classes(out, cnt, max_per_img, input_size=INPUT_SIZE):
        """One image's `out [nc,K,6]` / `cnt [nc]` (numpy) -> [n,6] rows: mmdet multiclass_nms's best `max_per_img` over all
        classes, by score (stable: class, then NMS order), boxes normalised to [0, 1]."""
        nc = out.shape[0]
        rows = np.concatenate([out[c, :cnt[c]] for c in range(nc)]) if cnt.sum() else np.zeros((0, 6), np.float32)
        order = np.argsort(-rows[:, 4], kind='stable')[:max_per_img]
        rows = rows[order]
        rows[:, :4] /= input_size
        return rows

    @torch.no_grad()
    def detect(self, imgs):
        out, cnt = self.detect_device(imgs)
        out, cnt = out.cpu().numpy(), cnt.cpu().numpy()
        return [self.merge_classes(out[b], cnt[b], self.max_per_img) for b in range(out.shape[0])]
